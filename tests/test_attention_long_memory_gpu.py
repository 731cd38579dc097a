"""GPU: cross-attention over visual memories of more than 128 keys (three / four modalities, long clips) -- the streaming
kernels of attn_mfma.hpp (fwd_stream_kernel, bwd_kb_stream_kernel) through the C ABI, against float64 references of the same
arithmetic, and continuity with the kernels that serve memories of up to 128 keys."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

H, DK = 8, 64
D = H * DK


def _ops():
    import nacf_amd  # noqa: F401
    from nacf_amd.runtime import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _heads(x, L):
    return x.view(x.shape[0], L, H, DK).permute(0, 2, 1, 3)


def _mha_ref(q, k, v):
    """q [R, Lq, D], k / v [R, Lk, D] (gathered per sequence), no mask; returns o [R, Lq, D] and p [H, R, Lq, Lk]"""
    R, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    p = torch.softmax(_heads(q, Lq) @ _heads(k, Lk).transpose(-1, -2) / math.sqrt(DK), -1)
    return (p @ _heads(v, Lk)).permute(0, 2, 1, 3).reshape(R, Lq, D), p.permute(1, 0, 2, 3)


def _case(Bv, k_, Lq, Lk, mode):
    R = Bv * k_
    vid = (torch.arange(R) % Bv) if mode == "mod" else (torch.arange(R) // k_)
    kv_div, kv_mod = (1, Bv) if mode == "mod" else (k_, Bv)
    return R, vid, kv_div, kv_mod, rnd(R * Lq, D, seed=1), rnd(Bv * Lk, 2 * D, seed=2), rnd(R * Lq, D, seed=3)


def _fwd(ops, dev, q, kv, R, Lq, Lk, kv_div, kv_mod, probs=None):
    out = torch.full((R * Lq, D), float("nan"), device=dev)
    ops.attention_fwd(q, kv[:, :D], kv[:, D:], out, None, 0, probs, R, H, Lq, Lk, DK, kv_div, kv_mod)
    return out


def _bwd(ops, dev, q, kv, do, R, Bv, Lq, Lk, kv_div, kv_mod):
    dq, dkv = torch.full_like(q, float("nan")), torch.full_like(kv, float("nan"))
    ops.attention_bwd(q, kv[:, :D], kv[:, D:], do, dq, dkv[:, :D], dkv[:, D:], None, 0, R, Bv, H, Lq, Lk, DK, kv_div, kv_mod)
    return dq, dkv


@pytest.mark.parametrize("mode", ["mod", "div"])
@pytest.mark.parametrize("Lk", [129, 144, 180, 240, 300])
def test_long_memory_forward_backward_against_float64_autograd(dev, mode, Lk):
    """H = 8, dk = 64, Lq = 20, two sequences per memory in both row maps; the last key block ragged (129: one live key);
    the bars of the model-width test at 120 keys; outputs pre-filled with NaN; a second call returns the same bits"""
    ops = _ops()
    Bv, k_, Lq = 5, 2, 20
    R, vid, kv_div, kv_mod, q, kv, do = _case(Bv, k_, Lq, Lk, mode)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    o_ref, _ = _mha_ref(qd.view(R, Lq, D), kvd[:, :D].reshape(Bv, Lk, D)[vid], kvd[:, D:].reshape(Bv, Lk, D)[vid])
    o_ref.backward(do.view(R, Lq, D).double())
    qx, kvx, dox = q.to(dev), kv.to(dev), do.to(dev)
    out = _fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod)
    dq, dkv = _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    assert err(out, o_ref.reshape(R * Lq, D)) < 5e-5
    assert err(dq, qd.grad) < 5e-5 and err(dkv, kvd.grad) < 1e-4
    out2 = _fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod)
    dq2, dkv2 = _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    assert torch.equal(out, out2) and torch.equal(dq, dq2) and torch.equal(dkv, dkv2)     # no atomics, fixed orders


def test_long_memory_backward_sums_many_sequences_per_memory(dev):
    """six sequences per memory (the "div" map of a length beam) and a ragged batch: the last memory has fewer sequences"""
    ops = _ops()
    Bv, k_, Lq, Lk = 3, 6, 32, 180
    R = Bv * k_ - 2
    vid = torch.arange(R) // k_
    q, kv, do = rnd(R * Lq, D, seed=1), rnd(Bv * Lk, 2 * D, seed=2), rnd(R * Lq, D, seed=3)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    o_ref, _ = _mha_ref(qd.view(R, Lq, D), kvd[:, :D].reshape(Bv, Lk, D)[vid], kvd[:, D:].reshape(Bv, Lk, D)[vid])
    o_ref.backward(do.view(R, Lq, D).double())
    qx, kvx = q.to(dev), kv.to(dev)
    out = _fwd(ops, dev, qx, kvx, R, Lq, Lk, k_, Bv)
    dq, dkv = _bwd(ops, dev, qx, kvx, do.to(dev), R, Bv, Lq, Lk, k_, Bv)
    assert err(out, o_ref.reshape(R * Lq, D)) < 5e-5
    assert err(dq, qd.grad) < 5e-5 and err(dkv, kvd.grad) < 2e-4      # six terms per memory row where the bar above sums two


@pytest.mark.parametrize("Lk", [180, 240])
@pytest.mark.parametrize("L", [19, 29])
def test_merged_candidates_equal_the_per_candidate_call(dev, L, Lk):
    """decode: the length-beam candidates of a video as ONE sequence of lbs * L queries (114 and 174: more than four blocks of
    32 queries, i.e. two groups of items per workgroup) -- the same bits as one sequence per candidate; attention maps on request"""
    ops = _ops()
    Bv, lbs = 3, 6
    R = Bv * lbs
    q, kv = rnd(R * L, D, seed=1).to(dev), rnd(Bv * Lk, 2 * D, seed=2).to(dev)
    vid = torch.arange(R) // lbs
    o_ref, p_ref = _mha_ref(q.cpu().double().view(R, L, D), kv.cpu()[:, :D].double().view(Bv, Lk, D)[vid],
                            kv.cpu()[:, D:].double().view(Bv, Lk, D)[vid])
    per = _fwd(ops, dev, q, kv, R, L, Lk, lbs, Bv)
    assert err(per, o_ref.reshape(R * L, D)) < 5e-5
    merged = _fwd(ops, dev, q, kv, Bv, lbs * L, Lk, 1, Bv)
    assert torch.equal(per, merged)
    probs = torch.full((H, Bv, lbs * L, Lk), float("nan"), device=dev)
    with_maps = _fwd(ops, dev, q, kv, Bv, lbs * L, Lk, 1, Bv, probs=probs)
    assert torch.equal(per, with_maps)
    assert float((probs.sum(-1) - 1).abs().max()) < 1e-5
    assert err(probs.view(H, Bv, lbs, L, Lk), p_ref.reshape(H, Bv, lbs, L, Lk)) < 1e-6


def test_memories_of_128_keys_keep_their_kernels(dev, monkeypatch):
    """the dispatch boundary: at 128 keys nothing changes with the streaming kernels switched off, at 129 keys switching them
    off restores the refusal of the backward"""
    ops = _ops()
    Bv, k_, Lq = 4, 2, 20
    res = {}
    for stream in (None, "0"):
        if stream is not None:
            monkeypatch.setenv("NACF_ATTN_STREAM", stream)
        R, vid, kv_div, kv_mod, q, kv, do = _case(Bv, k_, Lq, 128, "mod")
        qx, kvx = q.to(dev), kv.to(dev)
        res[stream] = (_fwd(ops, dev, qx, kvx, R, Lq, 128, kv_div, kv_mod),) + _bwd(ops, dev, qx, kvx, do.to(dev), R, Bv, Lq, 128,
                                                                                  kv_div, kv_mod)
    assert all(torch.equal(a, b) for a, b in zip(res[None], res["0"]))
    R, vid, kv_div, kv_mod, q, kv, do = _case(Bv, k_, Lq, 129, "mod")
    with pytest.raises(RuntimeError, match="Lk\\*dk <= 8192"):
        _bwd(ops, dev, q.to(dev), kv.to(dev), do.to(dev), R, Bv, Lq, 129, kv_div, kv_mod)


@pytest.mark.parametrize("Lk", [120, 70, 33])
def test_streaming_kernels_on_a_short_memory_agree_with_the_one_block_kernels(dev, Lk, monkeypatch):
    """NACF_ATTN_STREAM=2 sends memories of 33..128 keys to the streaming kernels too: the same quantities in another summation
    order (running statistics over 64-key blocks; dQ over chunks), equal to 1e-6"""
    ops = _ops()
    Bv, k_, Lq = 4, 2, 20
    R, vid, kv_div, kv_mod, q, kv, do = _case(Bv, k_, Lq, Lk, "div")
    qx, kvx, dox = q.to(dev), kv.to(dev), do.to(dev)
    old = (_fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod),) + _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    monkeypatch.setenv("NACF_ATTN_STREAM", "2")
    new = (_fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod),) + _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    for a, b in zip(old, new):
        assert err(a, b) < 1e-6
    if Lk > 64:
        assert not torch.equal(old[0], new[0])                   # it IS another kernel (two key blocks: another summation order)


def _bf(x):
    return x.float().to(torch.bfloat16).double()


def _stream_bf16_restatement(q, k, v, do, block):
    """The throughput mode of the streaming kernels in float64: every matrix-instruction operand rounded to bf16, everything else
    in full precision.  Forward: per block of `block` keys the UNNORMALISED probabilities exp(S - running maximum) are the rounded
    operand of P V, the accumulator is rescaled when the maximum rises and divided by the (unrounded) sum at the end.  Backward:
    the normalised P and dS are the rounded operands, as in the one-block kernels."""
    R, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    qh, kh, vh, doh = _heads(q, Lq), _heads(k, Lk), _heads(v, Lk), _heads(do, Lq)
    s = _bf(qh) @ _bf(kh).transpose(-1, -2) / math.sqrt(DK)
    m = torch.full(s.shape[:-1] + (1,), -float("inf"), dtype=torch.float64)
    acc = torch.zeros(R, H, Lq, DK, dtype=torch.float64)
    for k0 in range(0, Lk, block):
        sb = s[..., k0:k0 + block]
        m_new = torch.maximum(m, sb.max(-1, keepdim=True).values)
        acc = acc * torch.exp(m - m_new) + _bf(torch.exp(sb - m_new)) @ _bf(vh[:, :, k0:k0 + block])
        m = m_new
    o = acc / torch.exp(s - m).sum(-1, keepdim=True)
    p = torch.softmax(s, -1)
    dp = _bf(doh) @ _bf(vh).transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) / math.sqrt(DK)
    back = lambda x, L: x.permute(0, 2, 1, 3).reshape(R, L, D)
    return (back(o, Lq), back(_bf(ds) @ _bf(kh), Lq), back(_bf(ds).transpose(-1, -2) @ _bf(qh), Lk),
            back(_bf(p).transpose(-1, -2) @ _bf(doh), Lk))


@pytest.mark.parametrize("Lk,k_", [(180, 2), (240, 6)])
def test_long_memory_with_bf16_operands_equals_its_rounding_restatement(dev, Lk, k_, monkeypatch):
    """NACF_ATTN_BF16=1 (the default of the bf16 GEMM mode).  Bars as in the 120-key test: what one bf16 rounding of a P / dS
    element on a rounding boundary can move (the kernel's fp32 soft-max and the restatement's differ in the last bits), far below
    the distance to the unrounded result.  The measured errors are printed (pytest -s)."""
    monkeypatch.setenv("NACF_ATTN_BF16", "1")
    ops = _ops()
    Bv, Lq = 4, 20
    R, vid, kv_div, kv_mod, q, kv, do = _case(Bv, k_, Lq, Lk, "div")
    kk, vv = kv[:, :D].reshape(Bv, Lk, D)[vid].double(), kv[:, D:].reshape(Bv, Lk, D)[vid].double()
    o_ref, dq_ref, dk_seq, dv_seq = _stream_bf16_restatement(q.view(R, Lq, D).double(), kk, vv, do.view(R, Lq, D).double(), 64)
    dk_ref = torch.zeros(Bv, Lk, D, dtype=torch.float64).index_add_(0, vid, dk_seq)
    dv_ref = torch.zeros(Bv, Lk, D, dtype=torch.float64).index_add_(0, vid, dv_seq)
    o_exact, _ = _mha_ref(q.view(R, Lq, D).double(), kk, vv)
    qx, kvx, dox = q.to(dev), kv.to(dev), do.to(dev)
    out = _fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod)
    dq, dkv = _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    e_o = err(out.view(R, Lq, D), o_ref)
    print("bf16 long memory Lk=%d: out %.2e (to exact %.2e) dq %.2e dk %.2e dv %.2e" % (
        Lk, e_o, err(out.view(R, Lq, D), o_exact), err(dq.view(R, Lq, D), dq_ref),
        err(dkv[:, :D].reshape(Bv, Lk, D), dk_ref), err(dkv[:, D:].reshape(Bv, Lk, D), dv_ref)))
    assert e_o < 1e-3, e_o
    assert err(out.view(R, Lq, D), o_exact) > 4 * e_o            # it IS the bf16 form
    assert err(dq.view(R, Lq, D), dq_ref) < 2e-3
    assert err(dkv[:, :D].reshape(Bv, Lk, D), dk_ref) < 4e-3 and err(dkv[:, D:].reshape(Bv, Lk, D), dv_ref) < 4e-3
    dq2, dkv2 = _bwd(ops, dev, qx, kvx, dox, R, Bv, Lq, Lk, kv_div, kv_mod)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    monkeypatch.setenv("NACF_ATTN_BF16", "0")                    # the switch is per call: fp32 operands again
    assert err(_fwd(ops, dev, qx, kvx, R, Lq, Lk, kv_div, kv_mod).view(R, Lq, D), o_exact) < 2e-5


def test_probability_dropout_over_a_long_memory_names_its_limit(dev):
    """attention_probs_dropout_prob > 0 stays on the LDS-tile kernels: beyond their tile the error says which limit and why"""
    ops = _ops()
    Bv, Lq, Lk = 2, 174, 180
    q, kv = rnd(Bv * Lq, D, seed=1).to(dev), rnd(Bv * Lk, 2 * D, seed=2).to(dev)
    out = torch.empty_like(q)
    with pytest.raises(RuntimeError, match="attention_probs_dropout_prob"):
        ops.attention_fwd(q, kv[:, :D], kv[:, D:], out, None, 0, None, Bv, H, Lq, Lk, DK, 1, Bv, drop=(0.1, 7, ops.RngState(1, dev)))


# ------------------------------------------------------------------ model level: three modalities, long clips
def _long_memory_opt(modality, n_frames, **more):
    import nacf_amd
    return nacf_amd.opts.make_opt("NACF", "MSRVTT", with_category=True, modality=modality, dim_a=128, n_frames=n_frames, max_len=20,
                                  vocab_size=1200, fused_loss=True, hidden_dropout_prob=0.0, encoder_dropout=0.0, **more)


def _batch(b, dev):
    return {"feats": [f.to(dev) for f in b["feats"]], "tokens": b["tokens"].to(dev), "tokens_1": b["tokens_1"].to(dev),
            "labels": b["labels"].to(dev), "labels_1": b["labels_1"].to(dev), "category": b["category"].to(dev),
            "length_target": b["tgt_length"].to(dev)}


@pytest.mark.parametrize("modality,n_frames", [("ami", 60), ("mi", 72)])
def test_three_modality_model_trains_and_decodes_like_the_oracle(dev, modality, n_frames):
    """NACF at d = 512, 8 heads, B = 8 with a visual memory of 180 keys (audio + motion + image, 60 frames) and of 144 keys (72
    frames): one training step (loss, encoder outputs, every gradient) against the CPU oracle; the step replayed from a hipGraph
    equals the launch-by-launch step; mask-predict decoding with coarse-grained templates and a length beam of 6, graph on and
    off, returns the oracle's tokens on rows without a near-tie.  Before the streaming kernels the first backward of this model
    failed with NACF_EUNSUPPORTED."""
    import nacf_amd
    from nacf_amd import synthetic as S
    from nacf_amd.misc.crit import get_criterion
    from nacf_amd.misc.optim import get_optimizer
    from nacf_amd.models.Translator import Translator
    from oracle import nacf_oracle as O
    opt = _long_memory_opt(modality, n_frames)
    M = len(modality) * n_frames
    sd = S.init_state_dict(opt, seed=0)
    b = S.synth_batch(opt, 8, n_frames, seed=11)
    model = nacf_amd.get_model(opt)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model.to(dev).train()
    crit, optim = get_criterion(model.opt), get_optimizer(model.opt, model)
    optim.zero_grad()
    res = model(feats=[f.to(dev) for f in b["feats"]], tgt_tokens=[b["tokens_1"].to(dev), b["tokens"].to(dev)],
                category=b["category"].to(dev))
    res["tgt_word_labels"] = [b["labels_1"].to(dev), b["labels"].to(dev)]
    res["tgt_length"] = b["tgt_length"].to(dev)
    loss = crit.get_loss(res)
    loss.backward()
    o_loss, _, o_grads = O.train_step({k: v.clone() for k, v in sd.items()}, opt, b["feats"], [b["tokens_1"], b["tokens"]],
                                      b["category"], [b["labels_1"], b["labels"]], b["tgt_length"], {}, lr=opt["learning_rate"])
    assert abs(float(loss) - float(o_loss)) <= 1e-5 * abs(float(o_loss)), (float(loss), float(o_loss))
    for k, p in model.named_parameters():
        scale = float(o_grads[k].abs().max())
        if scale <= 1e-7:
            assert float(p.grad.abs().max()) < 1e-5, k
            continue
        assert err(p.grad, o_grads[k]) <= 2e-4 * scale, (k, err(p.grad, o_grads[k]) / scale)

    # encoder outputs and NA decoding against the oracle (a fresh model: the training forward moved the BatchNorm running statistics)
    model = nacf_amd.get_model(opt)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model.to(dev).eval()
    feats, cat = [f.to(dev) for f in b["feats"]], b["category"].to(dev)
    o_enc = O.encode(sd, opt, b["feats"], training=False)
    assert o_enc["enc_output"].shape == (8, M, 512)
    dec = dict(paradigm="mp", use_ct=True, iterations=5, length_beam_size=6, beam_alpha=1.35)
    o_hyp, *_ = O.generate(sd, opt, dec, o_enc, b["category"])
    hyps = {}
    for graph in ("off", "on"):
        with torch.no_grad():
            enc = model.encode(feats=feats)
        assert err(enc["enc_output"], o_enc["enc_output"]) < 2e-4 and err(enc["pred_length"], o_enc["pred_length"]) < 2e-4
        hyps[graph], _ = Translator(model, dict(model.opt, decode_graph=graph, **dec), device=dev).translate_batch(enc, cat, None, None)
    assert torch.equal(hyps["on"], hyps["off"])
    assert torch.equal(hyps["off"].cpu(), o_hyp), (hyps["off"].cpu(), o_hyp)     # (no near-tie among these eight videos)


def test_three_modality_step_replayed_from_a_graph_equals_launch_by_launch(dev):
    from nacf_amd import synthetic as S
    from nacf_amd.misc.crit import get_criterion
    from nacf_amd.misc.optim import get_optimizer
    from nacf_amd.misc.run import get_forword_results
    from nacf_amd.runtime.engine import TrainStep
    import nacf_amd
    opt = _long_memory_opt("ami", 60)
    batches = [_batch(S.synth_batch(opt, 8, 60, seed=20 + s), dev) for s in range(3)]
    out = {}
    for graph in ("off", "on"):
        model = nacf_amd.get_model(opt)
        model.load_state_dict(S.init_state_dict(opt, seed=0))
        model.to(dev).train()
        crit, optim = get_criterion(model.opt), get_optimizer(model.opt, model)
        engine = TrainStep(model, crit, optim, lambda bb, m=model: get_forword_results(m.opt, m, bb, dev), graph=graph)
        losses = []
        for bb in batches + batches[:1]:
            engine(bb)
            losses.append(float(engine.loss))
        out[graph] = (model.flat.data.clone(), losses)
        assert engine.captured == (graph == "on")
    assert out["on"][1] == out["off"][1] and all(l == l for l in out["on"][1])
    assert torch.equal(out["on"][0], out["off"][0])
