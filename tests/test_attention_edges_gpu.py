"""GPU: the attention kernels where uniform random inputs never reach -- sharp soft-max ranges, fully masked rows, shape and mask
edges -- through the C ABI against the float64 reference of tests/attn_cases.py, WITH THE DISPATCHED KERNEL ASSERTED BY NAME
(nacf_attention_last_kernel).  Outputs are pre-filled with NaN and live inside larger buffers whose guard rows and columns hold a
sentinel that must be bit-unchanged afterwards.  Error bars: attn_cases.bars, per element (derived there, not tuned).

Kernel -> the dispatch inputs that select it (csrc/nacf_decoder.hip, nacf_attention_fwd_dropout / _bwd_dropout; every operand
16-byte aligned with ld % 4 == 0, NACF_ATTN_VALU unset, no probability dropout; PR = NACF_ATTN_BF16, else the bf16 GEMM mode, dk = 64):

  forward
    fwd_stream_kernel<4, PR, probs|no probs>   dk = 64, Lk > 128, no key mask, not causal, any Lq
    fwd_lds_kernel<4, PR>                      dk = 64, 32 < Lk <= 128, no key mask, not causal, no probs,
                                               (sequences per memory) * ceil(Lq / 32) >= 4, NACF_ATTN_LDS != 0
    fwd_kernel<2, 1|4, PR>                     dk = 16 | 64, Lk <= 32 (Lq <= 32 if causal, else blocks of 32 queries)
    fwd_kernel<8, 1|4, PR>                     dk = 16 | 64, 32 < Lk <= 128 and not taken by fwd_lds_kernel
    attention_fwd_kernel                       everything else: unaligned operands, other dk, causal with Lq > 32, NACF_ATTN_VALU=1
  backward
    bwd_kb_stream_kernel<4, PR>                dk = 64, Lk > 128, no key mask, not causal, Lq <= 32
    bwd_kb_kernel<4> | <4, 1, 1> (PR)          dk = 64, 32 < Lk <= 128, no key mask, not causal, Lq <= 32, NACF_ATTN_KB != 0
    bwd_kb_kernel<4, 0>                        the same with NACF_ATTN_KB=2 (the guarded-load form)
    bwd_kernel<2|8, 1|4, PR> wpi=1|2|4         dk = 16 | 64, Lq <= 32, Lk <= 32 | <= 128 and not taken by bwd_kb_kernel;
                                               wpi = NACF_ATTN_WPI when the memory serves at least that many sequences
    attention_bwd_kernel                       everything else (needs Lk * dk <= 8192)

The last test prints the coverage the module reached: kernel name -> passing cases per profile / mask group.
Wall time on one MI355X: 294 cases in 60 s (dominated by the float64 references on the host)."""
import os
import time

import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
GUARD_ROWS, GUARD_COLS = 3, 4
COVERAGE = {}            # (kernel, group) -> passing cases
ATTEMPTED, PLANNED = set(), set()
T0 = []                  # when the first test of this module started


def _ops():
    import nacf_amd  # noqa: F401
    from nacf_amd.runtime import ops
    return ops


@pytest.fixture(autouse=True)
def _stream_switch_not_leaked():
    """tests/conftest.py guards the tuning variables it lists; NACF_ATTN_STREAM is not on that list and decides which kernels every
    case below runs on"""
    assert "NACF_ATTN_STREAM" not in os.environ, "NACF_ATTN_STREAM leaked into this test"
    if not T0:
        T0.append(time.time())
    yield


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


class Guarded:
    """a [rows, width] output filled with NaN inside a [GUARD_ROWS + rows + GUARD_ROWS, width + guard columns] buffer of SENTINEL"""

    def __init__(self, rows, width, dev, guard_cols=GUARD_COLS, col0=0):
        self.buf = torch.full((rows + 2 * GUARD_ROWS, col0 + width + guard_cols), SENTINEL, device=dev)
        self.rows, self.width, self.col0 = rows, width, col0
        self.view = self.buf[GUARD_ROWS:GUARD_ROWS + rows, col0:col0 + width]
        self.view.fill_(float("nan"))

    def cols(self, a, b):
        return self.view[:, a:b]

    def assert_guard_untouched(self, what):
        g = self.buf.clone()
        g[GUARD_ROWS:GUARD_ROWS + self.rows, self.col0:self.col0 + self.width] = SENTINEL
        same = torch.equal(g.view(torch.int32), torch.full_like(g, SENTINEL).view(torch.int32))
        assert same, "%s: a write outside the live region (guard rows / columns changed)" % what


def _note(kernel, group):
    COVERAGE[(kernel, group)] = COVERAGE.get((kernel, group), 0) + 1


def run_case(dev, monkeypatch, *, profile, kind, R, Lq, H, dk, Lk=None, n_mem=None, k_=1, key_pad=None, causal=0, bf16=False,
             env=None, want_fwd=None, want_bwd=None, probs=False, misalign=None, group=None, seed=0, inputs=None, check=True):
    """One case through the C ABI: build the inputs (Q / K / V as column slices of packed buffers, as the model passes them), call
    forward and backward twice each, assert the kernel names, the guards, run-to-run equality and the results against float64.
    kind: "self" (Lk = Lq, one memory per sequence, packed [rows, 3D]) | "mod" | "div" (row maps onto n_mem shared memories,
    K / V packed [rows, 2D]).  want_bwd=None: no backward.  Returns the device results."""
    with monkeypatch.context() as mp:          # the switches of this case end with it
        for name, value in dict(env or {}).items():
            mp.setenv(name, value)
        mp.setenv("NACF_ATTN_BF16", "1" if bf16 else "0")          # whatever --gemm-mode the session runs under
        return _run_case(dev, profile, kind, R, Lq, H, dk, Lk, n_mem, k_, key_pad, causal, bf16, want_fwd, want_bwd, probs, misalign,
                         group, seed, inputs, check)


def _run_case(dev, profile, kind, R, Lq, H, dk, Lk, n_mem, k_, key_pad, causal, bf16, want_fwd, want_bwd, probs, misalign, group, seed,
              inputs, check):
    ops = _ops()
    D = H * dk
    if kind == "self":
        Lk, n_mem = Lq, R
        vid, kv_div, kv_mod = torch.arange(R), 1, R
    else:
        vid, kv_div, kv_mod = A.row_map(R, kind, k_, n_mem)
    q, k, v, do, info = inputs if inputs is not None else A.make_inputs(profile, R, n_mem, Lq, Lk, H, dk, seed=seed)
    long_rows = Lk >= 100
    n_terms = int(torch.bincount(vid, minlength=n_mem).max())
    stream = (want_fwd or "").startswith("fwd_stream")
    ref = A.reference(q, k, v, do, vid, n_mem, R, Lq, Lk, H, key_pad=key_pad, causal=causal, bf16=bf16, block=64 if stream else None) \
        if check else None
    # ---- device operands
    if kind == "self":
        x = torch.cat([q, k, v], 1).to(dev)
        qx, kx, vx = x[:, :D], x[:, D:2 * D], x[:, 2 * D:]
    else:
        qx = q.to(dev)
        kvx = torch.cat([k, v], 1).to(dev)
        kx, vx = kvx[:, :D], kvx[:, D:]
    if misalign == "ld":          # a leading dimension that is not a multiple of 4 floats
        kx = torch.cat([kx, torch.zeros(kx.shape[0], 3, device=dev)], 1)[:, :D]
        assert kx.stride(0) % 4 != 0
    elif misalign == "base":      # a base pointer 4 bytes off a 16-byte boundary
        kx = torch.cat([torch.zeros(kx.shape[0], 1, device=dev), kx, torch.zeros(kx.shape[0], 3, device=dev)], 1)[:, 1:1 + D]
        assert kx.data_ptr() % 16 != 0 and kx.stride(0) % 4 == 0
    tok = None
    if key_pad is not None:
        tok = torch.where(key_pad, torch.full(key_pad.shape, A.PAD), torch.full(key_pad.shape, 7)).to(torch.int64).to(dev)
    dox = do.to(dev)
    res = {}
    for rep in range(2):
        out = Guarded(R * Lq, D, dev)
        pr = Guarded(H * R * Lq, Lk, dev, guard_cols=0) if probs else None
        ops.attention_fwd(qx, kx, vx, out.view, tok, causal, pr.view.view(H, R, Lq, Lk) if probs else None, R, H, Lq, Lk, dk, kv_div,
                          kv_mod)
        name_f = ops.attention_last_kernel()
        assert name_f == want_fwd, "forward ran on %r, expected %r" % (name_f, want_fwd)
        out.assert_guard_untouched("O")
        cur = {"o": out.view.clone()}
        if probs:
            pr.assert_guard_untouched("probs")
            cur["p"] = pr.view.view(H, R, Lq, Lk).clone()
        if want_bwd is not None:
            if kind == "self":
                g = Guarded(R * Lq, 3 * D, dev)
                dq, dk_, dv = g.cols(0, D), g.cols(D, 2 * D), g.cols(2 * D, 3 * D)
                guards = [(g, "dQ|dK|dV")]
            else:
                gq, gkv = Guarded(R * Lq, D, dev), Guarded(n_mem * Lk, 2 * D, dev)
                dq, dk_, dv = gq.view, gkv.cols(0, D), gkv.cols(D, 2 * D)
                guards = [(gq, "dQ"), (gkv, "dK|dV")]
            ops.attention_bwd(qx, kx, vx, dox, dq, dk_, dv, tok, causal, R, n_mem, H, Lq, Lk, dk, kv_div, kv_mod)
            name_b = ops.attention_last_kernel()
            assert name_b == want_bwd, "backward ran on %r, expected %r" % (name_b, want_bwd)
            for gd, what in guards:
                gd.assert_guard_untouched(what)
            cur.update(dq=dq.clone(), dk=dk_.clone(), dv=dv.clone())
        if rep == 0:
            res = cur
        else:
            for name in cur:        # fixed combination orders: a second call returns the same bits (NaN included)
                assert torch.equal(cur[name].view(torch.int32), res[name].view(torch.int32)), "run-to-run: %s differs" % name
    if not check:
        return res
    bar = A.bars(ref, profile, bf16=bf16, long_rows=long_rows, n_terms=n_terms)
    for name in res:
        kern = want_fwd if name in ("o", "p") else want_bwd
        assert torch.isfinite(res[name]).all(), "%s holds NaN / Inf (%s, %s)" % (name, profile, kern)
        diff = (res[name].double().cpu() - ref[name]).abs()
        over = diff / bar[name]                      # per element: the bar is a tensor shaped like the output
        worst = int(over.argmax())
        assert float(over.max()) < 1.0, "%s: element %d is off by %.3e, its bar is %.3e (%s; %s; largest |reference| %.3e)" % (
            name, worst, float(diff.flatten()[worst]), float(bar[name].flatten()[worst]), profile, kern, float(ref[name].abs().max()))
    grp = group or profile
    _note(want_fwd, grp)
    if want_bwd is not None:
        _note(want_bwd, grp)
    res["ref"] = ref
    return res


# ---------------------------------------------------------------- every kernel x every score profile
MFMA8 = {"NACF_ATTN_KB": "0", "NACF_ATTN_LDS": "0"}
FAMILIES = {
    # self-attention (one memory per sequence), Lq = Lk <= 32
    "self16": dict(kind="self", R=5, Lq=17, H=4, dk=16, want=("fwd_kernel<2, 1, 0>", "bwd_kernel<2, 1, 0> wpi=1")),
    "self64": dict(kind="self", R=3, Lq=31, H=8, dk=64, want=("fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=1")),
    "self64_bf16": dict(kind="self", R=3, Lq=32, H=8, dk=64, bf16=True, want=("fwd_kernel<2, 4, 1>", "bwd_kernel<2, 4, 1> wpi=1")),
    # cross-attention, dk = 16: the one-wave-per-item kernels at any memory length up to 128; R is not a multiple of k_ * n_mem
    "cross16": dict(kind="div", R=7, k_=3, n_mem=3, Lq=16, Lk=65, H=4, dk=16, want=("fwd_kernel<8, 1, 0>", "bwd_kernel<8, 1, 0> wpi=1")),
    "cross16_wpi2": dict(kind="div", R=7, k_=3, n_mem=3, Lq=31, Lk=128, H=4, dk=16, env={"NACF_ATTN_WPI": "2"},
                         want=("fwd_kernel<8, 1, 0>", "bwd_kernel<8, 1, 0> wpi=2")),
    # cross-attention, dk = 64, a memory of up to 32 keys; 3 / 5 sequences per memory
    "short64": dict(kind="mod", R=7, n_mem=3, Lq=17, Lk=32, H=8, dk=64, want=("fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=1")),
    "short64_wpi2": dict(kind="mod", R=7, n_mem=3, Lq=32, Lk=17, H=8, dk=64, env={"NACF_ATTN_WPI": "2"},
                         want=("fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=2")),
    "short64_wpi4": dict(kind="div", R=13, k_=5, n_mem=3, Lq=16, Lk=31, H=4, dk=64, env={"NACF_ATTN_WPI": "4"},
                         want=("fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=4")),
    # cross-attention, dk = 64, 33..128 keys: three sequences per memory keep the forward off the LDS-staged kernel
    "kb": dict(kind="mod", R=5, n_mem=2, Lq=20, Lk=127, H=8, dk=64, want=("fwd_kernel<8, 4, 0>", "bwd_kb_kernel<4>")),
    "kb_guarded": dict(kind="mod", R=5, n_mem=2, Lq=31, Lk=65, H=8, dk=64, env={"NACF_ATTN_KB": "2"},
                       want=("fwd_kernel<8, 4, 0>", "bwd_kb_kernel<4, 0>")),
    "kb_bf16": dict(kind="mod", R=5, n_mem=2, Lq=20, Lk=128, H=8, dk=64, bf16=True, want=("fwd_kernel<8, 4, 1>", "bwd_kb_kernel<4, 1, 1>")),
    # ... six per memory put it on fwd_lds_kernel (the last memory serves four)
    "lds": dict(kind="div", R=16, k_=6, n_mem=3, Lq=19, Lk=120, H=8, dk=64, want=("fwd_lds_kernel<4, 0>", "bwd_kb_kernel<4>")),
    "lds_bf16": dict(kind="div", R=16, k_=6, n_mem=3, Lq=19, Lk=97, H=8, dk=64, bf16=True,
                     want=("fwd_lds_kernel<4, 1>", "bwd_kb_kernel<4, 1, 1>")),
    # ... and with the key-block / LDS kernels switched off, the one-wave-per-item kernels at NKT = 8, 1 / 2 / 4 waves per memory
    "mfma8": dict(kind="div", R=16, k_=6, n_mem=3, Lq=19, Lk=120, H=8, dk=64, env=MFMA8,
                  want=("fwd_kernel<8, 4, 0>", "bwd_kernel<8, 4, 0> wpi=1")),
    "mfma8_wpi2": dict(kind="div", R=16, k_=6, n_mem=3, Lq=32, Lk=33, H=8, dk=64, env=dict(MFMA8, NACF_ATTN_WPI="2"),
                       want=("fwd_kernel<8, 4, 0>", "bwd_kernel<8, 4, 0> wpi=2")),
    "mfma8_wpi4": dict(kind="div", R=16, k_=6, n_mem=3, Lq=17, Lk=64, H=8, dk=64, env=dict(MFMA8, NACF_ATTN_WPI="4"),
                       want=("fwd_kernel<8, 4, 0>", "bwd_kernel<8, 4, 0> wpi=4")),
    "mfma8_bf16": dict(kind="div", R=16, k_=6, n_mem=3, Lq=19, Lk=120, H=8, dk=64, env=MFMA8, bf16=True,
                       want=("fwd_kernel<8, 4, 1>", "bwd_kernel<8, 4, 1> wpi=1")),
    # more than 128 keys: the streaming kernels
    "stream": dict(kind="div", R=5, k_=2, n_mem=3, Lq=20, Lk=193, H=8, dk=64,
                   want=("fwd_stream_kernel<4, 0, no probs>", "bwd_kb_stream_kernel<4, 0>")),
    "stream_probs": dict(kind="mod", R=5, n_mem=2, Lq=32, Lk=300, H=8, dk=64, probs=True,
                         want=("fwd_stream_kernel<4, 0, probs>", "bwd_kb_stream_kernel<4, 0>")),
    "stream_bf16": dict(kind="div", R=5, k_=2, n_mem=3, Lq=20, Lk=257, H=8, dk=64, bf16=True,
                        want=("fwd_stream_kernel<4, 1, no probs>", "bwd_kb_stream_kernel<4, 1>")),
    "stream_bf16_probs": dict(kind="div", R=5, k_=2, n_mem=3, Lq=17, Lk=192, H=8, dk=64, bf16=True, probs=True,
                              want=("fwd_stream_kernel<4, 1, probs>", "bwd_kb_stream_kernel<4, 1>")),
    # NACF_ATTN_STREAM=2 sends 33..128 keys there too (one and two blocks of 64 keys)
    "stream_short": dict(kind="div", R=5, k_=2, n_mem=3, Lq=20, Lk=127, H=8, dk=64, env={"NACF_ATTN_STREAM": "2"},
                         want=("fwd_stream_kernel<4, 0, no probs>", "bwd_kb_stream_kernel<4, 0>")),
    # the LDS / VALU kernels
    "generic16": dict(kind="self", R=5, Lq=17, H=4, dk=16, env={"NACF_ATTN_VALU": "1"}, want=("attention_fwd_kernel", "attention_bwd_kernel")),
    "generic64": dict(kind="div", R=7, k_=3, n_mem=3, Lq=20, Lk=120, H=8, dk=64, env={"NACF_ATTN_VALU": "1"},
                      want=("attention_fwd_kernel", "attention_bwd_kernel")),
    "generic24": dict(kind="mod", R=5, n_mem=2, Lq=9, Lk=40, H=2, dk=24, want=("attention_fwd_kernel", "attention_bwd_kernel")),
}
for _f in FAMILIES:
    for _p in A.PROFILES:
        PLANNED.add("%s-%s" % (_f, _p))


def _family_case(dev, monkeypatch, family, profile, **over):
    f = dict(FAMILIES[family])
    want = f.pop("want")
    f.update(over)
    return run_case(dev, monkeypatch, profile=profile, want_fwd=want[0], want_bwd=want[1], probs=f.pop("probs", True), **f)


@pytest.mark.parametrize("profile", A.PROFILES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_on_every_score_profile(dev, monkeypatch, family, profile):
    """forward (with the returned probabilities where the kernel stores them), backward, names, guards, run-to-run equality"""
    ATTEMPTED.add("%s-%s" % (family, profile))
    f = FAMILIES[family]
    probs = f.get("probs", not f["want"][0].startswith(("fwd_lds", "fwd_stream")))      # asking for probs moves those kernels
    _family_case(dev, monkeypatch, family, profile, probs=probs)


def test_sharp_and_twin_rows_are_what_the_profile_says(dev, monkeypatch):
    """the profiles reach the kernels as constructed: a sharp query puts P > 1 - 1e-9 on its winner (first / last key, tile, wave and
    block edges among them), twins share the mass equally to the last bit"""
    r = _family_case(dev, monkeypatch, "stream_probs", "sharp")
    _, _, _, _, info = A.make_inputs("sharp", 5, 2, 32, 300, 8, 64)
    win = info["winners"].to(r["p"].device)
    pw = r["p"].gather(-1, win.view(1, 5, 32, 1).expand(8, 5, 32, 1))
    assert float(pw.min()) > 1 - 1e-6 and {0, 299, 63, 64, 127, 128, 255, 256} <= set(win.flatten().tolist())
    for fam in ("stream_probs", "kb", "self16"):
        r = _family_case(dev, monkeypatch, fam, "twin")
        f = FAMILIES[fam]
        a, b = A.twin_keys(f.get("Lk", f["Lq"]))
        assert torch.equal(r["p"][..., a], r["p"][..., b]) and float((r["p"][..., a] - 0.5).abs().max()) < 1e-6


# ---------------------------------------------------------------- shape edges
ONE_BLOCK_LK = [1, 15, 16, 17, 32, 33, 63, 64, 65, 127, 128]
STREAM_LK = [129, 191, 192, 193, 256, 257, 300]
EDGE_LQ = [1, 16, 17, 31, 32]
EDGE_PROFILES = ["sharp", "rising", "twin", "falling"]


def _cross64_names(Lk, Lq, nseq):
    if Lk > 128:
        return "fwd_stream_kernel<4, 0, no probs>", "bwd_kb_stream_kernel<4, 0>"
    if Lk > 32:
        return ("fwd_lds_kernel<4, 0>" if nseq * ((Lq + 31) // 32) >= 4 else "fwd_kernel<8, 4, 0>"), "bwd_kb_kernel<4>"
    return "fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=1"


@pytest.mark.parametrize("i,Lk", list(enumerate(ONE_BLOCK_LK + STREAM_LK)))
def test_memory_length_edges_dk64(dev, monkeypatch, i, Lk):
    """cross-attention at dk = 64 over every memory length where a tile, a wave's key share, a block or a kernel ends; query counts,
    row maps and sequences per memory (1, 2, 3, 5, 6; the last memory short) rotate with it"""
    Lq, profile = EDGE_LQ[i % 5], EDGE_PROFILES[i % 4]
    if Lk == 1 and profile == "twin":
        profile = "sharp"
    kind, k_, n_mem, R = [("div", 2, 3, 5), ("mod", 1, 2, 5), ("div", 6, 3, 16), ("div", 5, 2, 9), ("mod", 1, 3, 3), ("div", 1, 3, 3)][i % 6]
    cdiv = lambda a, b: -(-a // b)
    nseq_max = k_ * cdiv(cdiv(R, k_), n_mem) if kind == "div" else cdiv(R, n_mem)      # sequences per memory, as the dispatch counts them
    fwd, bwd = _cross64_names(Lk, Lq, nseq_max)
    run_case(dev, monkeypatch, profile=profile, kind=kind, R=R, k_=k_, n_mem=n_mem, Lq=Lq, Lk=Lk, H=4, dk=64, want_fwd=fwd,
             want_bwd=bwd, group="edge:" + profile, seed=i)


@pytest.mark.parametrize("i,Lk", list(enumerate(ONE_BLOCK_LK)))
def test_memory_length_edges_dk16_and_one_wave_per_item_kernels(dev, monkeypatch, i, Lk):
    """dk = 16, and dk = 64 with the key-block / LDS kernels switched off: fwd_kernel / bwd_kernel at NKT = 2 and 8 on every edge"""
    Lq, profile = EDGE_LQ[(i + 2) % 5], EDGE_PROFILES[(i + 1) % 4]
    if Lk == 1 and profile == "twin":
        profile = "sharp"
    nkt = 2 if Lk <= 32 else 8
    run_case(dev, monkeypatch, profile=profile, kind="div", R=7, k_=3, n_mem=3, Lq=Lq, Lk=Lk, H=4, dk=16, probs=True,
             want_fwd="fwd_kernel<%d, 1, 0>" % nkt, want_bwd="bwd_kernel<%d, 1, 0> wpi=1" % nkt, group="edge:" + profile, seed=i)
    wpi = (1, 2, 4)[i % 3]
    env = dict(MFMA8, NACF_ATTN_WPI=str(wpi))
    run_case(dev, monkeypatch, profile=profile, kind="div", R=16, k_=6, n_mem=3, Lq=Lq, Lk=Lk, H=4, dk=64, env=env, probs=True,
             want_fwd="fwd_kernel<%d, 4, 0>" % nkt, want_bwd="bwd_kernel<%d, 4, 0> wpi=%d" % (nkt, wpi), group="edge:" + profile, seed=i)


@pytest.mark.parametrize("Lq", [33, 64, 65, 96])
def test_forward_blocks_of_32_queries(dev, monkeypatch, Lq):
    """more than 32 queries per sequence: the forward kernels walk blocks of 32 (the backward kernels stop at 32: not called)"""
    common = dict(kind="div", R=5, k_=2, n_mem=3, Lq=Lq, H=4, want_bwd=None)
    run_case(dev, monkeypatch, profile="sharp", Lk=31, dk=64, probs=True, want_fwd="fwd_kernel<2, 4, 0>", group="Lq>32", **common)
    run_case(dev, monkeypatch, profile="rising", Lk=128, dk=64, probs=True, want_fwd="fwd_kernel<8, 4, 0>", group="Lq>32", **common)
    run_case(dev, monkeypatch, profile="twin", Lk=100, dk=16, probs=True, want_fwd="fwd_kernel<8, 1, 0>", group="Lq>32", **common)
    run_case(dev, monkeypatch, profile="rising", Lk=65, dk=64, want_fwd="fwd_lds_kernel<4, 0>", group="Lq>32", **common)
    run_case(dev, monkeypatch, profile="sharp", Lk=257, dk=64, want_fwd="fwd_stream_kernel<4, 0, no probs>", group="Lq>32", **common)
    run_case(dev, monkeypatch, profile="falling", Lk=192, dk=64, probs=True, want_fwd="fwd_stream_kernel<4, 0, probs>", group="Lq>32", **common)


# ---------------------------------------------------------------- masks
def _key_pad(R, Lk, seed=0):
    """sequence 0 all <pad>; 1 only the first key live; 2 only the last; 3 <pad> on both sides of every tile / wave / block edge;
    the rest a padded tail of random length"""
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(R, Lk, dtype=torch.bool)
    pad[0] = True
    if R > 1:
        pad[1, 1:] = True
    if R > 2:
        pad[2, :-1] = True
    if R > 3:
        for kk in (15, 16, 31, 32, 63, 64, 127):
            if kk < Lk - 1:
                pad[3, kk] = True
    for r in range(4, R):
        pad[r, int(torch.randint(1, Lk + 1, (1,), generator=g)):] = True
    return pad


def _assert_all_pad_sequence(res, v, do, vid, Lq, Lk, D, tol):
    """sequence 0, every key <pad>: P uniform 1 / Lk over ALL keys, O the mean of V, dQ EXACTLY 0 and nothing added to dK
    (masked_fill passes no gradient, models/bert.py:160); P still feeds dV"""
    p0 = res["p"][:, 0]
    assert float((p0 - 1.0 / Lk).abs().max()) < 1e-7
    m = int(vid[0])
    vmean = v.view(-1, Lk, D)[m].double().mean(0)
    assert err(res["o"][:Lq], vmean.expand(Lq, D)) < tol
    assert bool((res["dq"][:Lq] == 0).all()), "dQ of a fully masked sequence: max |dQ| = %.3e" % float(res["dq"][:Lq].abs().max())


MASK_FAMILIES = {
    "self16": dict(kind="self", R=6, Lq=17, H=4, dk=16, want=("fwd_kernel<2, 1, 0>", "bwd_kernel<2, 1, 0> wpi=1")),
    "self64": dict(kind="self", R=5, Lq=32, H=8, dk=64, want=("fwd_kernel<2, 4, 0>", "bwd_kernel<2, 4, 0> wpi=1")),
    "self64_bf16": dict(kind="self", R=5, Lq=31, H=8, dk=64, bf16=True, want=("fwd_kernel<2, 4, 1>", "bwd_kernel<2, 4, 1> wpi=1")),
    # a key mask on cross-attention geometry with 33..128 keys: NKT = 8 with key tokens, the second ballot word for keys 64..127
    "cross16_128": dict(kind="div", R=7, k_=3, n_mem=3, Lq=17, Lk=128, H=4, dk=16, want=("fwd_kernel<8, 1, 0>", "bwd_kernel<8, 1, 0> wpi=1")),
    "cross64_65": dict(kind="div", R=7, k_=3, n_mem=3, Lq=16, Lk=65, H=8, dk=64, want=("fwd_kernel<8, 4, 0>", "bwd_kernel<8, 4, 0> wpi=1")),
    "cross64_128_wpi2": dict(kind="mod", R=7, n_mem=3, Lq=31, Lk=128, H=4, dk=64, env={"NACF_ATTN_WPI": "2"},
                             want=("fwd_kernel<8, 4, 0>", "bwd_kernel<8, 4, 0> wpi=2")),
    "cross64_33_bf16": dict(kind="mod", R=7, n_mem=3, Lq=20, Lk=33, H=4, dk=64, bf16=True, want=("fwd_kernel<8, 4, 1>", "bwd_kernel<8, 4, 1> wpi=1")),
    "generic16": dict(kind="self", R=6, Lq=17, H=4, dk=16, env={"NACF_ATTN_VALU": "1"}, want=("attention_fwd_kernel", "attention_bwd_kernel")),
    "generic64": dict(kind="div", R=7, k_=3, n_mem=3, Lq=20, Lk=127, H=8, dk=64, env={"NACF_ATTN_VALU": "1"},
                      want=("attention_fwd_kernel", "attention_bwd_kernel")),
    # more than 128 keys with a key mask: no streaming kernel takes a mask (dk = 16 keeps the tile inside the generic backward)
    "generic16_long": dict(kind="mod", R=5, n_mem=2, Lq=9, Lk=150, H=2, dk=16, want=("attention_fwd_kernel", "attention_bwd_kernel")),
}


@pytest.mark.parametrize("profile", ["uniform", "sharp", "all_low"])
@pytest.mark.parametrize("family", list(MASK_FAMILIES))
def test_key_masks_and_fully_masked_sequences(dev, monkeypatch, family, profile):
    f = dict(MASK_FAMILIES[family])
    want = f.pop("want")
    Lk = f.get("Lk", f["Lq"])
    pad = _key_pad(f["R"], Lk, seed=3)
    r = run_case(dev, monkeypatch, profile=profile, key_pad=pad, probs=True, want_fwd=want[0], want_bwd=want[1], group="key mask", **f)
    D = f["H"] * f["dk"]
    n_mem = f["R"] if f["kind"] == "self" else f["n_mem"]
    vid = torch.arange(f["R"]) if f["kind"] == "self" else A.row_map(f["R"], f["kind"], f.get("k_", 1), n_mem)[0]
    _, _, v, do, _ = A.make_inputs(profile, f["R"], n_mem, f["Lq"], Lk, f["H"], f["dk"])
    _assert_all_pad_sequence(r, v, do, vid, f["Lq"], Lk, D, 1e-2 if f.get("bf16") else 1e-5)
    if f["kind"] == "self":      # its own memory: nothing at all reaches dK, and dV = sum_q dO / Lk
        assert bool((r["dk"][:Lk] == 0).all())
        assert err(r["dv"][:Lk], (do[:f["Lq"]].double().sum(0) / Lk).expand(Lk, D)) < (2e-2 if f.get("bf16") else 1e-5)
    # partly masked rows: exactly no probability at a filled key
    assert float(r["p"][:, 1, :, 1:].abs().max()) == 0.0 and float(r["p"][:, 2, :, :-1].abs().max()) == 0.0


@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("dk,H", [(16, 4), (64, 8)])
@pytest.mark.parametrize("L", [1, 17, 32])
def test_causal_and_watch_windows(dev, monkeypatch, L, dk, H, valu):
    """causal = 1 and causal = w + 1 for watch windows w in {1, 2, 5, L}, alone and with a key mask (a padded tail: queries whose
    window holds nothing but <pad> are fully masked rows)"""
    dk16 = dk // 16
    want = ("attention_fwd_kernel", "attention_bwd_kernel") if valu else \
        ("fwd_kernel<2, %d, 0>" % dk16, "bwd_kernel<2, %d, 0> wpi=1" % dk16)
    env = {"NACF_ATTN_VALU": "1"} if valu else {}
    R = 4
    for n, w in enumerate([0, 1, 2, 5, L]):
        profile = ("uniform", "sharp", "rising", "all_high", "twin")[n]
        if L == 1 and profile == "twin":
            profile = "uniform"
        for pad in (None, _key_pad(R, L, seed=n) if L > 1 else None):
            if pad is not None:
                pad[0] = False
                pad[0, L // 2:] = True          # (not the all-<pad> sequence here: a padded tail under a window)
            run_case(dev, monkeypatch, profile=profile, kind="self", R=R, Lq=L, H=H, dk=dk, causal=1 + w, key_pad=pad, probs=True,
                     env=env, want_fwd=want[0], want_bwd=want[1], group="causal/watch", seed=n)


@pytest.mark.parametrize("geom", ["self", "cross"])
def test_probability_dropout_with_a_fully_masked_sequence(dev, geom):
    """attention_probs_dropout_prob > 0 runs the LDS / VALU kernels: sequence 0 with every key <pad> gets dQ exactly 0 and adds
    nothing to dK there too (its own memory: dK exactly 0; a shared memory: dK equals the call without sequence 0's dO ... which
    is the same thing as dK being unchanged when that sequence's Q is replaced), while the other sequences are untouched"""
    ops = _ops()
    H, dk, Lq, p, salt = 4, 16, 9, 0.3, 77
    D = H * dk
    if geom == "self":
        R, Lk, n_mem, kv_div, kv_mod = 4, Lq, 4, 1, 4
    else:
        R, Lk, n_mem, kv_div, kv_mod = 6, 40, 3, 2, 3
    q, k, v, do, _ = A.make_inputs("peaked", R, n_mem, Lq, Lk, H, dk, seed=2)
    pad = _key_pad(R, Lk, seed=1)
    tok = torch.where(pad, torch.full(pad.shape, A.PAD), torch.full(pad.shape, 7)).to(dev)

    def bwd(qq):
        dq, dk_, dv = [torch.full(x.shape, float("nan"), device=dev) for x in (q, k, v)]
        ops.attention_bwd(qq.to(dev), k.to(dev), v.to(dev), do.to(dev), dq, dk_, dv, tok, 0, R, n_mem, H, Lq, Lk, dk, kv_div, kv_mod,
                          drop=(p, salt, ops.RngState(11, dev)))
        assert ops.attention_last_kernel() == "attention_bwd_kernel"
        return dq, dk_, dv

    dq, dk_, dv = bwd(q)
    assert torch.isfinite(dq).all() and torch.isfinite(dk_).all() and torch.isfinite(dv).all()
    assert bool((dq[:Lq] == 0).all()), "dQ of a fully masked sequence under dropout: max %.3e" % float(dq[:Lq].abs().max())
    assert float(dq[Lq:].abs().max()) > 1e-3
    if geom == "self":
        assert bool((dk_[:Lk] == 0).all()) and float(dv[:Lk].abs().max()) > 1e-3
    q2 = q.clone()
    q2[:Lq] = A.rnd(Lq, D, seed=9)                  # other queries for the masked sequence: nothing else may move
    dq2, dk2, dv2 = bwd(q2)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk_) and torch.equal(dv2, dv)
    _note("attention_bwd_kernel", "dropout")


def test_causal_beyond_32_queries_takes_the_generic_kernels(dev, monkeypatch):
    run_case(dev, monkeypatch, profile="sharp", kind="self", R=3, Lq=40, H=4, dk=16, causal=1, probs=True,
             want_fwd="attention_fwd_kernel", want_bwd="attention_bwd_kernel", group="causal/watch")


# ---------------------------------------------------------------- fall-throughs of the dispatch
@pytest.mark.parametrize("misalign", ["ld", "base"])
@pytest.mark.parametrize("family", ["self16", "kb", "short64"])
def test_unaligned_operands_land_on_the_generic_kernels_and_stay_right(dev, monkeypatch, family, misalign):
    _family_case(dev, monkeypatch, family, "uniform")                         # aligned: the matrix-core kernels
    f = dict(FAMILIES[family])
    f.pop("want")
    for profile in ("sharp", "rising"):
        run_case(dev, monkeypatch, profile=profile, misalign=misalign, probs=True, want_fwd="attention_fwd_kernel",
                 want_bwd="attention_bwd_kernel", group="unaligned", **f)


def test_silent_fall_throughs_are_visible_by_name(dev, monkeypatch):
    """the switches only take effect where their conditions hold: too few sequences per memory for NACF_ATTN_WPI, too few items
    for fwd_lds_kernel, a long memory with the streaming kernels off (forward: generic; backward: the documented refusal)"""
    f = dict(FAMILIES["kb"])
    f.pop("want")
    run_case(dev, monkeypatch, profile="sharp", env=dict(MFMA8, NACF_ATTN_WPI="4"), want_fwd="fwd_kernel<8, 4, 0>",
             want_bwd="bwd_kernel<8, 4, 0> wpi=1", group="fall-through", **f)           # 3 sequences per memory < 4
    lds = {k: v for k, v in FAMILIES["lds"].items() if k != "want"}
    run_case(dev, monkeypatch, profile="rising", probs=True, want_fwd="fwd_kernel<8, 4, 0>", want_bwd="bwd_kb_kernel<4>",
             group="fall-through", **lds)                                               # attention maps asked for
    s = {k: v for k, v in FAMILIES["stream"].items() if k != "want"}
    run_case(dev, monkeypatch, profile="rising", env={"NACF_ATTN_STREAM": "0"}, want_fwd="attention_fwd_kernel", want_bwd=None,
             group="fall-through", **s)
    with pytest.raises(RuntimeError, match="Lk\\*dk <= 8192"):
        run_case(dev, monkeypatch, profile="rising", env={"NACF_ATTN_STREAM": "0"}, want_fwd="attention_fwd_kernel",
                 want_bwd="attention_bwd_kernel", group="fall-through", **s)


# ---------------------------------------------------------------- isolation between sequences that share a workgroup
@pytest.mark.parametrize("family", ["lds", "kb_bf16", "stream", "stream_bf16", "stream_short", "mfma8_wpi2", "short64_wpi4"])
def test_a_nan_sequence_or_memory_touches_nothing_else(dev, monkeypatch, family):
    """fwd_lds, the key-block and the streaming kernels serve every sequence of a memory from one workgroup and read clamped rows
    "replaced by zero": poison the Q rows of one sequence (then the K / V rows of one memory) with NaN -- every other sequence's O
    and dQ, and dK / dV of every other memory, keep their bits"""
    f = dict(FAMILIES[family])
    want = f.pop("want")
    R, Lq, Lk, H, dk, n_mem = f["R"], f["Lq"], f["Lk"], f["H"], f["dk"], f["n_mem"]
    vid, _, _ = A.row_map(R, f["kind"], f.get("k_", 1), n_mem)
    inputs = A.make_inputs("rising", R, n_mem, Lq, Lk, H, dk, seed=9)
    clean = run_case(dev, monkeypatch, profile="rising", inputs=inputs, want_fwd=want[0], want_bwd=want[1], check=False, **f)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    # one sequence's queries (the last sequence of memory vid[1]: clamped / "replaced by zero" rows sit next to it)
    bad = int((vid == vid[1]).nonzero().max())
    q2 = inputs[0].clone()
    q2[bad * Lq:(bad + 1) * Lq] = float("nan")
    dirty = run_case(dev, monkeypatch, profile="rising", inputs=(q2,) + inputs[1:], want_fwd=want[0], want_bwd=want[1], check=False, **f)
    seq_ok = torch.ones(R, dtype=torch.bool)
    seq_ok[bad] = False
    rows_q = seq_ok.repeat_interleave(Lq).to(dev)
    mem_ok = torch.ones(n_mem, dtype=torch.bool)
    mem_ok[vid[bad]] = False
    rows_k = mem_ok.repeat_interleave(Lk).to(dev)
    assert torch.isnan(dirty["o"][~rows_q]).all() and torch.isnan(dirty["dq"][~rows_q]).all()
    assert same(dirty["o"][rows_q], clean["o"][rows_q]) and same(dirty["dq"][rows_q], clean["dq"][rows_q])
    assert same(dirty["dk"][rows_k], clean["dk"][rows_k]) and same(dirty["dv"][rows_k], clean["dv"][rows_k])
    # one memory's keys and values
    j = int(vid[bad])
    k2, v2 = inputs[1].clone(), inputs[2].clone()
    k2[j * Lk:(j + 1) * Lk] = float("nan")
    v2[j * Lk:(j + 1) * Lk] = float("nan")
    dirty = run_case(dev, monkeypatch, profile="rising", inputs=(inputs[0], k2, v2) + inputs[3:], want_fwd=want[0], want_bwd=want[1],
                     check=False, **f)
    rows_q = (vid != j).repeat_interleave(Lq).to(dev)
    assert same(dirty["o"][rows_q], clean["o"][rows_q]) and same(dirty["dq"][rows_q], clean["dq"][rows_q])
    assert same(dirty["dk"][rows_k], clean["dk"][rows_k]) and same(dirty["dv"][rows_k], clean["dv"][rows_k])
    _note(want[0], "isolation")
    _note(want[1], "isolation")


# ---------------------------------------------------------------- what the module reached
ALL_KERNELS = [
    "fwd_kernel<2, 1, 0>", "fwd_kernel<2, 4, 0>", "fwd_kernel<2, 4, 1>", "fwd_kernel<8, 1, 0>", "fwd_kernel<8, 4, 0>", "fwd_kernel<8, 4, 1>",
    "fwd_lds_kernel<4, 0>", "fwd_lds_kernel<4, 1>", "fwd_stream_kernel<4, 0, no probs>", "fwd_stream_kernel<4, 0, probs>",
    "fwd_stream_kernel<4, 1, no probs>", "fwd_stream_kernel<4, 1, probs>", "attention_fwd_kernel",
    "bwd_kernel<2, 1, 0> wpi=1", "bwd_kernel<2, 4, 0> wpi=1", "bwd_kernel<2, 4, 0> wpi=2", "bwd_kernel<2, 4, 0> wpi=4",
    "bwd_kernel<2, 4, 1> wpi=1", "bwd_kernel<8, 1, 0> wpi=1", "bwd_kernel<8, 1, 0> wpi=2", "bwd_kernel<8, 4, 0> wpi=1",
    "bwd_kernel<8, 4, 0> wpi=2", "bwd_kernel<8, 4, 0> wpi=4", "bwd_kernel<8, 4, 1> wpi=1",
    "bwd_kb_kernel<4>", "bwd_kb_kernel<4, 0>", "bwd_kb_kernel<4, 1, 1>", "bwd_kb_stream_kernel<4, 0>", "bwd_kb_stream_kernel<4, 1>",
    "attention_bwd_kernel",
]


# the kernels that take a mask / serve several sequences from one workgroup must also have met those groups
_ONE_WAVE = ["fwd_kernel<2, 1, 0>", "fwd_kernel<2, 4, 0>", "attention_fwd_kernel", "bwd_kernel<2, 1, 0> wpi=1", "bwd_kernel<2, 4, 0> wpi=1",
             "attention_bwd_kernel"]
REQUIRED_GROUPS = {
    "causal/watch": _ONE_WAVE,
    "key mask": _ONE_WAVE + ["fwd_kernel<2, 4, 1>", "fwd_kernel<8, 1, 0>", "fwd_kernel<8, 4, 0>", "fwd_kernel<8, 4, 1>",
                             "bwd_kernel<2, 4, 1> wpi=1", "bwd_kernel<8, 1, 0> wpi=1", "bwd_kernel<8, 4, 0> wpi=1",
                             "bwd_kernel<8, 4, 0> wpi=2", "bwd_kernel<8, 4, 1> wpi=1"],
    "isolation": ["fwd_lds_kernel<4, 0>", "fwd_stream_kernel<4, 0, no probs>", "fwd_stream_kernel<4, 1, no probs>", "fwd_kernel<8, 4, 1>",
                  "bwd_kb_kernel<4>", "bwd_kb_kernel<4, 1, 1>", "bwd_kb_stream_kernel<4, 0>", "bwd_kb_stream_kernel<4, 1>",
                  "bwd_kernel<8, 4, 0> wpi=2", "bwd_kernel<2, 4, 0> wpi=4"],
    "unaligned": ["attention_fwd_kernel", "attention_bwd_kernel"],
}


def test_zz_every_kernel_was_pinned_on_every_profile():
    """prints kernel -> passing cases per profile / group; every instantiation the dispatch can reach must have met every profile, and
    the mask / causal / isolation / unaligned groups the kernels they apply to.  It reads what the tests above recorded in this
    process, so it needs them to have run before it in the same process (file order); on a partial run it skips."""
    if not PLANNED <= ATTEMPTED:
        pytest.skip("a partial run of this module: the coverage table needs test_every_kernel_on_every_score_profile in full")
    groups = list(A.PROFILES) + sorted({g for _, g in COVERAGE} - set(A.PROFILES))
    short = lambda g: g.replace("edge:", "e:")[:9]
    lines = ["%-36s" % "kernel" + " ".join("%9s" % short(g) for g in groups)]
    for kern in ALL_KERNELS + sorted({k for k, _ in COVERAGE} - set(ALL_KERNELS)):
        lines.append("%-36s" % kern + " ".join("%9d" % COVERAGE.get((kern, g), 0) for g in groups))
    print("\nattention kernel coverage (passing cases)\n" + "\n".join(lines))
    print("module wall time so far: %.1f s" % (time.time() - T0[0]))
    assert not set(k for k, _ in COVERAGE) - set(ALL_KERNELS), "a kernel name this table does not know"
    empty = [(k, p) for k in ALL_KERNELS for p in A.PROFILES if not COVERAGE.get((k, p))]
    empty += [(k, g) for g, kernels in REQUIRED_GROUPS.items() for k in kernels if not COVERAGE.get((k, g))]
    assert not empty, "no passing case for: %s" % empty
