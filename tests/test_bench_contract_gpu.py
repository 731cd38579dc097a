"""GPU: bench.py keeps the driver's contract -- ONE JSON line, last on stdout, with the agreed keys."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_contract_line(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--no-compare",
                          "--no-loader", "--decode-batches", "2"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    d = json.loads(lines[-1])                       # the JSON object is the LAST line
    assert sum(1 for l in lines if l.lstrip().startswith("{")) == 1
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["unit"] == "videos/s" and d["value"] > 1000 and abs(d["value"] - 128 / d["ms_per_step"] * 1e3) < 0.01 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert 0.1 < r["frac"] < 1.0 and (r["traffic"] is None or r["traffic"] > 0)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "videos/s" and c["value"] > 0 and c["cores"] >= 1 and c["sample"]
    assert d["decode"]["captions_per_s"] > 100


def test_dump_outputs_of_the_last_timed_step_repeat_run_to_run(dev, tmp_path):
    """--dump-outputs: loss, parameters after the last timed step and the meters as fp32 / fp64 .npy, at most 64 MB in all, and
    -- seeded weights, batch and dropout stream -- the same bits from two runs with the same arguments; --steps sets how many
    steps ran before the dump (one step more moves the weights)"""
    import numpy as np

    def run(tag, steps):
        d = str(tmp_path / tag)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "2", "--no-compare",
                              "--no-loader", "--no-decode", "--no-cpu-baseline", "--dump-outputs", d],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.strip().splitlines() if l.strip()][-1])
        assert line["steps"] == steps
        return line, {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    line, a = run("a", 4)
    _, b = run("b", 4)
    _, c = run("c", 5)
    assert sorted(a) == ["loss", "loss_info", "params"]
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["params"].size == 1 << 23                  # the seeded sample of the ~18 M parameters
    assert abs(float(a["loss"][0]) - line["final_loss"]) < 1e-3
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert float(np.abs(a["params"] - c["params"]).max()) > 1e-5


def test_multi_rank_launch_sequence_with_one_rank_group(dev):
    """NACF_BENCH_FORCE_DIST=1 runs the N > 1 step (two backward graphs, bucketed RCCL all-reduces on their own stream,
    Adam per bucket) with a 1-rank process group: it must capture, and train exactly like the single-graph step"""
    def run(env_extra):
        env = dict(os.environ, **env_extra)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--no-compare",
                              "--no-loader", "--no-decode", "--no-cpu-baseline"], capture_output=True, text=True,
                             timeout=600, cwd=ROOT, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([l for l in out.stdout.strip().splitlines() if l.strip()][-1])
    single = run({})
    multi = run({"NACF_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29577"})
    assert multi["config"]["hipgraph"] is True and multi["config"]["overlapped_allreduce"] is True
    assert multi["config"]["gradient_buckets"] == 2 and single["config"]["gradient_buckets"] == 1
    assert multi["config"]["sync_bn"] is True and single["config"]["sync_bn"] is False
    # same training: the SyncBN path of a 1-rank group folds its statistics in another order (round-off only)
    assert abs(multi["final_loss"] - single["final_loss"]) < 2e-3
    nosync = run({"NACF_BENCH_FORCE_DIST": "1", "NACF_BENCH_SYNC_BN": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29578"})
    # (two backward stages = two weight-gradient groups with their own split counts: the same sums in another order.  The line
    #  prints four decimals; round 4 saw 88.9784 vs 88.9785 on some boxes and equal digits on others, so the bar is the one of
    #  the SyncBN comparison above, not equality)
    assert abs(nosync["final_loss"] - single["final_loss"]) < 2e-3 and nosync["config"]["sync_bn"] is False
    assert multi["value"] > 0.8 * single["value"]
    # the three-stage variant (the vocabulary projection's bucket leaves a stage earlier) stays selectable
    three = run({"NACF_BENCH_FORCE_DIST": "1", "NACF_DDP_STAGES": "3", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29579"})
    assert three["config"]["gradient_buckets"] == 3 and abs(three["final_loss"] - single["final_loss"]) < 2e-3
    # NACF_DDP_GRAPH_COLLECTIVES=1: the RCCL calls captured INSIDE one step graph -- the same training, bit for bit
    one = run({"NACF_BENCH_FORCE_DIST": "1", "NACF_DDP_GRAPH_COLLECTIVES": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29580"})
    assert one["config"]["hipgraph"] is True and one["final_loss"] == multi["final_loss"]
    assert one["config"].get("graph_collectives") is True and not multi["config"].get("graph_collectives")


def test_forced_collective_sequences_yield_the_single_process_weights(dev, tmp_path):
    """What a final loss printed to four decimals would not notice (a bucket that skipped its Adam walk, a stage whose gradients
    were reduced twice): the POST-STEP WEIGHTS of the N > 1 launch sequences -- two and three gradient buckets with SyncBN, and
    the RCCL calls captured inside one step graph -- against the single-process step.  1-rank RCCL group, dropout 0, 3 steps
    (one launch by launch, two replayed); SyncBN folds its statistics in another order and the staged backward groups the
    weight-gradient GEMMs differently, so the bar is round-off: max |dw| <= 1e-5 on weights of O(0.1)."""
    import torch
    helper = os.path.join(ROOT, "tests", "ddp_step_helper.py")

    def run(tag, kind, port, **env_extra):
        path = str(tmp_path / (tag + ".pt"))
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **env_extra)
        out = subprocess.run([sys.executable, helper, path, kind, "3"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        return torch.load(path, weights_only=True)
    single = run("single", "single", 29590)
    assert single["captured"] and single["buckets"] == 1
    w0 = single["weights"]
    for tag, env, buckets, in_graph in (("two", {}, 2, False), ("three", {"NACF_DDP_STAGES": "3"}, 3, False),
                                        ("ingraph", {"NACF_DDP_GRAPH_COLLECTIVES": "1"}, None, True)):
        r = run(tag, "dist", 29591 + len(tag), **env)
        assert r["captured"], tag
        if buckets is not None:
            assert r["staged"] and r["buckets"] == buckets, (tag, r["buckets"])
        assert r["graph_collectives"] == in_graph, tag
        err = float((r["weights"] - w0).abs().max())
        assert err <= 1e-5, (tag, err)
        assert abs(r["loss"] - single["loss"]) <= 1e-4 * abs(single["loss"]), (tag, r["loss"], single["loss"])
    # ... and the steps did move the weights (three Adam steps at the schedule's learning rate)
    import nacf_amd
    from nacf_amd import synthetic as S
    opt = nacf_amd.opts.make_opt("NACF", "MSRVTT", with_category=True, max_len=20, vocab_size=1001, n_frames=12, fused_loss=True,
                                 hidden_dropout_prob=0.0, encoder_dropout=0.0, use_ct=True)
    m = nacf_amd.get_model(opt)
    m.load_state_dict(S.init_state_dict(opt, 0))
    m.to(dev)
    assert float((m.flat.data.cpu() - w0).abs().max()) > 1e-4
