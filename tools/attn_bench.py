"""Cross-attention kernel times at the training and the decode geometry for visual memories of 120, 180 and 240 keys (GPU box only).

usage: python tools/attn_bench.py [--out DIR] [--iters 20]

The driver starts ONE profiled child (`rocprofv3 --kernel-trace --stats ... -- python tools/attn_bench.py --workload`), which
launches every configuration `3 + iters` times in a fixed order and writes that order next to the trace; the driver then walks the
attention dispatches of the kernel trace in order and prints, per configuration, the kernel that served it and the median
microseconds per launch.  Geometries (d = 512, 8 heads of 64):
  train   B = 128 videos x two NACF passes ("mod" row map: 256 sequences), Lq = 20; forward and backward
  decode  B = 128 videos, the 6 length-beam candidates of a video merged into one sequence of 6 x 19 = 114 queries; forward
each with fp32 operands and with bf16 operands (NACF_ATTN_BF16), plus the kernels a long memory had before the streaming
kernels (NACF_ATTN_STREAM=0: the LDS / VALU kernel where its tile fits) and the streaming kernels forced onto 120 keys (=2)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, DK, D, B = 8, 64, 512, 128
WARM = 3


def plan():
    """(label, direction, R, Lq, M, bf16, NACF_ATTN_STREAM or None)"""
    out = []
    for M in (120, 180, 240):
        for bf in (0, 1):
            out.append(("train fwd", "fwd", 2 * B, 20, M, bf, None))
            out.append(("train bwd", "bwd", 2 * B, 20, M, bf, None))
            out.append(("decode fwd", "fwd", B, 6 * 19, M, bf, None))
    for bf in (0, 1):                                    # the streaming kernels on the memory the one-block kernels serve
        out.append(("train fwd", "fwd", 2 * B, 20, 120, bf, "2"))
        out.append(("train bwd", "bwd", 2 * B, 20, 120, bf, "2"))
        out.append(("decode fwd", "fwd", B, 6 * 19, 120, bf, "2"))
    out.append(("train fwd", "fwd", 2 * B, 20, 180, 0, "0"))          # before: the LDS / VALU kernel (its tile fits at 180 keys)
    out.append(("decode fwd", "fwd", B, 6 * 19, 180, 0, "0"))
    out.append(("train fwd", "fwd", 2 * B, 20, 240, 0, "0"))
    return out


def workload(iters, plan_path):
    sys.path.insert(0, ROOT)
    import torch
    import nacf_amd  # noqa: F401
    from nacf_amd.runtime import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1)).to(dev)
    done = []
    for label, direction, R, Lq, M, bf, stream in plan():
        q, kv, do = rnd(R * Lq, D), rnd(B * M, 2 * D), rnd(R * Lq, D)
        out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
        os.environ["NACF_ATTN_BF16"] = str(bf)
        if stream is None:
            os.environ.pop("NACF_ATTN_STREAM", None)
        else:
            os.environ["NACF_ATTN_STREAM"] = stream
        torch.cuda.synchronize()
        for _ in range(WARM + iters):
            if direction == "fwd":
                ops.attention_fwd(q, kv[:, :D], kv[:, D:], out, None, 0, None, R, H, Lq, M, DK, 1, B)
            else:
                ops.attention_bwd(q, kv[:, :D], kv[:, D:], do, dq, dkv[:, :D], dkv[:, D:], None, 0, R, B, H, Lq, M, DK, 1, B)
        torch.cuda.synchronize()
        done.append(dict(label=label, M=M, bf16=bf, stream=stream, launches=WARM + iters))
    json.dump(done, open(plan_path, "w"))


def short(name):
    for a in ("(anonymous namespace)::", "void ", "attn::"):
        name = name.replace(a, "")
    return name.split("(")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "attn_bench"))      # build/ is ignored by git
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--plan", default=None)
    a = ap.parse_args()
    if a.workload:
        return workload(a.iters, a.plan)
    os.makedirs(a.out, exist_ok=True)
    plan_path = os.path.join(a.out, "plan.json")
    subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out, "-o", "attn", "--",
                           sys.executable, os.path.abspath(__file__), "--workload", "--iters", str(a.iters), "--plan", plan_path],
                          stdout=subprocess.DEVNULL)
    trace = glob.glob(os.path.join(a.out, "**", "attn_kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(trace)))
    col = {c.lower(): c for c in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rows = [r for r in rows if "attn::" in r[name] or "attention_fwd_kernel" in r[name] or "attention_bwd_kernel" in r[name]]
    rows.sort(key=lambda r: int(r[t0]))
    done = json.load(open(plan_path))
    assert len(rows) == sum(c["launches"] for c in done), (len(rows), sum(c["launches"] for c in done))
    lines = ["cross-attention kernels, B = 128, d = 512, 8 heads x 64: median us per launch over %d launches (kernel trace)" % a.iters,
             "%-11s %4s  %-5s %-9s %9s   %s" % ("geometry", "M", "PR", "STREAM", "us", "kernel")]
    at = 0
    for c in done:
        mine = rows[at:at + c["launches"]]
        at += c["launches"]
        names = {short(r[name]) for r in mine}
        assert len(names) == 1, names
        us = statistics.median((int(r[t1]) - int(r[t0])) / 1e3 for r in mine[WARM:])
        lines.append("%-11s %4d  %-5s %-9s %9.1f   %s" % (c["label"], c["M"], "bf16" if c["bf16"] else "fp32",
                                                          "default" if c["stream"] is None else "=" + c["stream"], us, names.pop()))
    text = "\n".join(lines)
    print(text)
    open(os.path.join(a.out, "attn_long_memory.txt"), "w").write(text + "\n")


if __name__ == "__main__":
    main()
