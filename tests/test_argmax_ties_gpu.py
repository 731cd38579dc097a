"""GPU: EXACT ties in the argmax paths under the bit-exact decode claim.  Continuous random data never ties, so the documented
"smallest index on ties" of the vocabulary argmax epilogues (gemm_f32.hpp:argmax_epilogue, the EpiArgmax forms of gemm_bf16.hpp /
gemm_dma128.hpp, argmax_merge_kernel across column tiles), of nacf_vocab_logsoftmax_fwd / nacf_vocab_lse_fwd, of the length beam
and of the candidate selection had never been run.  Ties are built, not hoped for: duplicated weight rows (and biases) give
bit-identical logits, because every output column accumulates over K in the same order wherever its tile lies
(attn_cases.duplicate_rows; its CPU check is in test_attention_refs_cpu.py).  Expected: what torch.max does on the CPU for the
same duplicated matrix -- the first maximal index -- and a log-sum-exp that counts both twins."""
import pytest
import torch

import attn_cases as A

pytestmark = pytest.mark.gpu

PAD, MASK = 0, 4
BODIES = set()           # GEMM kernels the tie cases ran on


def _ops():
    import nacf_amd  # noqa: F401
    from nacf_amd.runtime import ops
    return ops


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def tie_pairs(V):
    """(first, twin) columns: inside one 16-column MFMA tile, across wave tiles, across workgroup column tiles of width 64, 128 and
    256, the first and the last column, and -- at the full vocabulary -- the ragged last tile"""
    pairs = [(3, 5), (15, 16), (17, 40), (60, 70), (63, 64), (0, V - 1)]
    if V > 300:
        pairs += [(120, 130), (127, 128), (250, 260), (255, 256), (1, V - 40), (V - 4, V - 2), (5000, V - 3)]
    return pairs


def tied_problem(rows, V, K, seed=0):
    """hidden [rows, K], w [V, K], bias [V]: row r's maximum logit is shared, to the bit, by the two columns of pair r % n.  Coordinate j
    of the hidden state is reserved for pair j (16 in the rows of that pair, 0 elsewhere; 8 in both twin weight rows, 0 elsewhere):
    +128 on the twins over logits of at most about 20."""
    pairs = tie_pairs(V)
    n = len(pairs)
    h, w, b = A.rnd(rows, K, seed=seed + 1), A.rnd(V, K, seed=seed + 2, scale=0.5), A.rnd(V, seed=seed + 3)
    h[:, :n] = 0.0
    w[:, :n] = 0.0
    for j, (a, _) in enumerate(pairs):
        w[a, j] = 8.0
    for r in range(rows):
        h[r, r % n] = 16.0
    A.duplicate_rows(w, b, pairs)                     # the twin becomes a copy of the first occurrence ...
    first = torch.tensor([pairs[r % n][0] for r in range(rows)])
    twin = torch.tensor([pairs[r % n][1] for r in range(rows)])
    return h, w, b, first, twin


def _tied_reference(h, w, b, first, twin):
    """float64 logits on the CPU.  A blocked float64 matmul need not accumulate two equal columns in the same order, so the twin's
    column is written as a copy of the first occurrence's: the reference then holds the exact tie the duplicated rows define."""
    z = h.double() @ w.double().t() + b.double()
    return z.scatter(1, twin.view(-1, 1), z.gather(1, first.view(-1, 1)))


STEER = [("f32", None), ("f32", "64"), ("f32", "128"), ("bf16x3", None), ("bf16x3", "64"), ("bf16x3", "128"), ("bf16", None),
         ("bf16", "64"), ("bf16", "128")]


def _steered(ops, monkeypatch, mode, tile, fn):
    """run fn() under a GEMM arithmetic mode (restored afterwards) and a forced tile; returns the GEMM kernel it launched"""
    before = ops.gemm_mode()
    if tile is not None:
        monkeypatch.setenv("NACF_GEMM_TILE", tile)
    try:
        ops.set_gemm_mode(mode)
        fn()
        name = ops.L.load().nacf_gemm_last_kernel().decode()
    finally:
        ops.set_gemm_mode(before)
    if mode == "f32":
        assert "bf16" not in name and "dma" not in name and "wide" not in name, name
    else:
        assert name.endswith("EpiArgmax>") and name.startswith(("gemm_bf16_kernel", "gemm_dma128_kernel", "gemm_dma64_kernel", "gemm_wide")), name
        if tile is not None and name.startswith("gemm_bf16_kernel"):
            assert name.startswith("gemm_bf16_kernel<%s, %s" % (tile, tile)), name
    BODIES.add(name)
    return name


@pytest.mark.parametrize("mode,tile", STEER)
@pytest.mark.parametrize("rows,V,K", [(57, 101, 64), (300, 10547, 512)])
def test_vocab_argmax_returns_the_first_of_two_bit_equal_maxima(dev, monkeypatch, rows, V, K, mode, tile):
    ops = _ops()
    h, w, b, first, twin = tied_problem(rows, V, K)
    z = _tied_reference(h, w, b, first, twin)
    assert torch.equal(torch.max(z, -1)[1], first)                                              # torch: the first maximal index
    pad = torch.full((rows,), 9)
    tok = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    pr = torch.full((rows,), -1.0, device=dev)
    hx, wx, bx = h.to(dev), w.to(dev), b.to(dev)
    _steered(ops, monkeypatch, mode, tile, lambda: ops.vocab_argmax(hx, wx, bx, pad.to(dev), False, None, tok, pr))
    wrong = (tok.cpu() != first).nonzero().flatten().tolist()
    assert not wrong, "rows %s: got %s, twins %s / %s" % (wrong[:8], tok.cpu()[wrong][:8].tolist(), first[wrong][:8].tolist(),
                                                        twin[wrong][:8].tolist())
    # both twins are in the soft-max sum: p(max) is close to 1/2, not to 1
    p_ref = torch.softmax(z, -1).max(-1)[0]
    assert err(pr, p_ref) < (2e-3 if mode == "bf16" else 2e-5) and float(pr.max()) < 0.51


@pytest.mark.parametrize("mode,tile", STEER)
@pytest.mark.parametrize("rows,V,K", [(70, 101, 64), (300, 10547, 512)])
def test_vocab_lse_fwd_ties_smallest_index_and_lse_counts_both_twins(dev, monkeypatch, rows, V, K, mode, tile):
    ops = _ops()
    h, w, b, first, twin = tied_problem(rows, V, K, seed=5)
    z = _tied_reference(h, w, b, first, twin)
    labels = torch.where(torch.arange(rows) % 3 == 0, twin, first)           # the label on either twin: same log-probability
    labels[labels == PAD] = 1
    live = ops.rowset_build(tokens=labels.to(dev))
    buf = torch.full((rows, ops.vocab_ld(V)), float("nan"), device=dev)
    logits = buf[:, :V]
    lse, llp = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
    am = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    hx, wx, bx = h.to(dev), w.to(dev), b.to(dev)
    _steered(ops, monkeypatch, mode, tile, lambda: ops.vocab_lse_fwd(hx, wx, bx, logits, labels.to(dev), lse, am, llp, live))
    got = logits.cpu()
    assert torch.equal(got.gather(1, first.view(-1, 1)), got.gather(1, twin.view(-1, 1))), "the twins' logits are not the same bits"
    assert torch.equal(am.cpu(), first)
    lse_ref = torch.logsumexp(z, 1)
    # the suite's 1e-4 holds for logits of a few units; the twins' logits are about 130 here (fp32 spacing 1.5e-5, K up to 512
    # terms): 16 times that.  One twin dropped from the sum would be ln 2 = 0.69
    tol = 5e-2 if mode == "bf16" else 1.6e-3
    assert err(lse, lse_ref) < tol
    assert err(llp, z.gather(1, labels.view(-1, 1)).squeeze(1) - lse_ref) < tol


@pytest.mark.parametrize("V", [101, 10547])
def test_vocab_logsoftmax_fwd_ties_smallest_index(dev, V):
    ops = _ops()
    rows = 64
    pairs = tie_pairs(V)
    z = A.rnd(rows, V, seed=1, scale=4)
    first = torch.tensor([pairs[r % len(pairs)][0] for r in range(rows)])
    twin = torch.tensor([pairs[r % len(pairs)][1] for r in range(rows)])
    z.scatter_(1, first.view(-1, 1), 9.0)
    z.scatter_(1, twin.view(-1, 1), 9.0)
    z[rows - 1] = 1.25                                                        # a whole row of equal logits: index 0
    first[rows - 1] = 0
    assert torch.equal(torch.max(z, -1)[1], first)
    labels = torch.randint(1, 9, (rows,), generator=torch.Generator().manual_seed(2))
    buf = torch.zeros(rows, ops.vocab_ld(V), device=dev)
    buf[:, :V] = z.to(dev)
    lse = torch.empty(rows, device=dev)
    am = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    ll = torch.empty(rows, device=dev)
    ops.vocab_logsoftmax_fwd(buf[:, :V], V, labels.to(dev), lse, am, ll)
    assert torch.equal(am.cpu(), first)
    assert err(lse, torch.logsumexp(z.double(), -1)) < 2e-5


def test_length_beam_orders_equal_lengths_by_ascending_index(dev):
    """nacf_length_beam documents "descending value, ascending index on ties".  The reference takes pred_length.topk(lbs)
    (decoding/na_generate.py:116-135; oracle/nacf_oracle.py:predict_length_beam), and torch leaves the order of equal elements
    unspecified: against the oracle only the selected SET is asserted, and only where the tie does not straddle position lbs; the
    order is asserted against the documented rule (a stable descending sort)."""
    from oracle import nacf_oracle as O
    ops = _ops()
    B, max_len, lbs = 6, 20, 6
    pl = torch.log_softmax(A.rnd(B, max_len, seed=1, scale=3), -1)
    pl[0, 7] = pl[0, 12] = pl[0].max() + 1.0                   # the two best tie
    pl[1, [5, 9, 14]] = pl[1].topk(3)[0][2]                     # three equal values inside the top six
    pl[2, [6, 8, 10, 16]] = pl[2].max() + 0.5                   # four equal best
    kth = pl[3].topk(lbs)[0][lbs - 1]
    pl[3, 17] = kth                                             # a tie that straddles position lbs: one of two equal values is cut
    pl[4, :] = -3.0                                             # every length equally likely
    straddles = torch.tensor([False, False, False, True, True, False])
    beam = torch.empty(B, lbs, dtype=torch.int32, device=dev)
    bmax = torch.empty(1, dtype=torch.int32, device=dev)
    ops.length_beam(pl.to(dev), lbs, 0, beam, bmax)
    rule = torch.sort(pl, dim=1, descending=True, stable=True)[1][:, :lbs].clamp(4, max_len - 1)
    assert torch.equal(beam.cpu().long(), rule), (beam.cpu().tolist(), rule.tolist())
    assert int(bmax) == int(rule.max())
    ref = O.predict_length_beam(pl, lbs, 0, max_len)
    for bi in range(B):
        if not bool(straddles[bi]):
            assert sorted(beam[bi].cpu().tolist()) == sorted(ref[bi].tolist()), bi


def test_best_candidate_takes_the_first_of_equal_scores(dev):
    """equal candidate scores (two candidates of a video with the same length and the same probabilities): the oracle's
    score.max(-1)[1] (oracle/nacf_oracle.py:generate, decoding/na_generate.py:72) is torch's first maximal index"""
    ops = _ops()
    B, lbs, Lp, alpha = 6, 6, 15, 1.35
    g = torch.Generator().manual_seed(0)
    beam = torch.randint(4, Lp + 1, (B, lbs), generator=g)
    probs = (torch.rand(B * lbs, Lp, generator=g) * 0.5 + 0.05).view(B, lbs, Lp)
    tokens = torch.randint(6, 99, (B * lbs, Lp), generator=g).view(B, lbs, Lp)
    twins = [(0, 1), (4, 5), (2, 5), (0, 5), (1, 3), (3, 4)]
    for b_, (i, j) in enumerate(twins):
        probs[b_, i, :] = 0.95                                 # the best score of the video ...
        beam[b_, j] = beam[b_, i]
        probs[b_, j] = probs[b_, i]                            # ... twice, under different tokens
    pad = torch.arange(Lp).view(1, 1, -1) >= beam.view(B, lbs, 1)
    probs[pad] = 1.0
    tokens[pad] = PAD
    score = probs.log().sum(-1) / beam.float() ** alpha
    best = score.max(-1)[1]
    assert best.tolist() == [i for i, _ in twins]
    assert all(float(score[b_, i]) == float(score[b_, j]) for b_, (i, j) in enumerate(twins))
    out = torch.empty(B, Lp, dtype=torch.int64, device=dev)
    bi = torch.empty(B, dtype=torch.int32, device=dev)
    cl = torch.empty(B * lbs, Lp, device=dev)
    ops.best_candidate(tokens.view(B * lbs, Lp).to(dev), probs.view(B * lbs, Lp).to(dev), None, beam.to(torch.int32).to(dev), alpha, B,
                       lbs, Lp, out, bi, cl)
    assert torch.equal(bi.cpu().long(), best)
    assert torch.equal(out.cpu(), tokens.gather(1, best.view(B, 1, 1).expand(B, 1, Lp)).squeeze(1))


def test_zz_the_tie_cases_ran_on_more_than_one_gemm_body():
    """prints the GEMM kernels the tie cases ran on; the fp32 body and at least two bf16-family bodies must be among them"""
    if not BODIES:
        pytest.skip("a partial run of this module")
    print("\nargmax tie cases ran on:\n  " + "\n  ".join(sorted(BODIES)))
    fam = {n.split("<")[0] for n in BODIES}
    assert len([n for n in BODIES if "EpiArgmax" in n]) >= 2 and len(fam) >= 2, sorted(BODIES)
