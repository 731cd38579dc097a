"""CPU (no GPU needed): the score-profile generator, the float64 attention reference and the tie constructor that the GPU
modules test_attention_edges_gpu.py / test_argmax_ties_gpu.py rely on are checked here, against the stated ranges and against the
oracle's attention (oracle/nacf_oracle.py:mha, masked_fill(-10e6)), so that a GPU run is not spent on debugging them."""
import math

import pytest
import torch

import attn_cases as A
from oracle import nacf_oracle as O


def _scores(q, k, vid, R, Lq, Lk, H, dk):
    D = H * dk
    qh = A.heads(q.double().view(R, Lq, D), H)
    kh = A.heads(k.double().view(-1, Lk, D)[vid], H)
    return qh @ kh.transpose(-1, -2) / math.sqrt(dk)          # [R, H, Lq, Lk]


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("Lk", [17, 128, 300])
def test_profiles_yield_the_stated_score_ranges(dk, Lk):
    H, R, n_mem, Lq = 4, 5, 2, 9
    vid, _, _ = A.row_map(R, "mod", 1, n_mem)
    lim = 1.6 if dk == 64 else 2.2            # what the noise coordinates add (sigma = 1/3 at any dk; bounds of these seeded draws)
    for profile in A.PROFILES:
        q, k, v, do, info = A.make_inputs(profile, R, n_mem, Lq, Lk, H, dk, seed=3)
        assert q.dtype == torch.float32 and q.shape == (R * Lq, H * dk) and k.shape == (n_mem * Lk, H * dk)
        s = _scores(q, k, vid, R, Lq, Lk, H, dk)
        assert torch.isfinite(s).all()
        if profile == "uniform":
            assert float(s.abs().max()) < lim
        elif profile in ("sharp", "peaked"):
            gap = A.SHARP if profile == "sharp" else A.PEAK
            win = info["winners"]
            assert (win >= 0).all() and len(set(win.flatten().tolist())) == min(len(A.winner_keys(Lk, dk)), Lq + R - 1)
            top = s.argmax(-1)
            assert torch.equal(top, win.view(R, 1, Lq).expand(R, H, Lq))
            rest = s.scatter(-1, top.unsqueeze(-1), -1e9).max(-1).values
            assert float((s.max(-1).values - rest).min()) > gap - 2 * lim           # one key at +30 (+5) over the rest
            for edge in (0, Lk - 1, 15, 16):
                if edge < Lk:
                    assert edge in win
        elif profile == "rising":
            for b0 in range(0, Lk - 63, 32):   # the maximum rises by >= 20 per full wave share of 32 keys (>= 40 per block of 64)
                nxt = s[..., b0 + 32:b0 + 64].max(-1).values
                assert float((nxt - s[..., b0:b0 + 32].max(-1).values).min()) >= 20.0 - 2 * lim
            assert float(s.abs().max()) < 11.0 * ((Lk - 1) // 16) + lim + 1e-9
        elif profile == "falling":
            first = s[..., :16].max(-1).values
            if Lk > 16:
                assert float((first - s[..., 16:].max(-1).values).min()) >= 110.0
                assert float(torch.exp((s[..., 16:] - first.unsqueeze(-1)).float()).max()) == 0.0     # underflows in fp32
        elif profile == "all_low":
            assert -95.0 <= float(s.min()) and float(s.max()) <= -80.0
        elif profile == "all_high":
            assert 80.0 <= float(s.min()) and float(s.max()) <= 95.0
        elif profile == "twin":
            a, b = info["twins"]
            assert a // 16 != b // 16 and (Lk <= 64 or a // 64 != b // 64)
            assert torch.equal(s[..., a], s[..., b])                                  # exactly equal maxima
            assert torch.equal(s.max(-1).values, s[..., a])
            kf = k.view(n_mem, Lk, -1)
            assert torch.equal(kf[:, a], kf[:, b])


def _oracle_mha(q, k, v, H, mask):
    """oracle/nacf_oracle.py:mha with identity projections: its masked soft-max attention on q / k / v as given"""
    D = q.shape[-1]
    sd = {}
    for n in ("query", "key", "value"):
        sd["a.self.%s.weight" % n] = torch.eye(D, dtype=q.dtype)
        sd["a.self.%s.bias" % n] = torch.zeros(D, dtype=q.dtype)
    opt = {"num_attention_heads": H, "attention_probs_dropout_prob": 0.0}
    return O.mha(sd, "a.", opt, q, k, mask, False, v_in=v)


@pytest.mark.parametrize("causal", [0, 1, 3])
@pytest.mark.parametrize("profile", ["uniform", "sharp", "all_low"])
def test_reference_equals_the_oracle_attention_with_masks(profile, causal):
    """key mask with one sequence all <pad>, one with only the first key live and one with only the last; causal and watch window;
    forward and autograd gradients in float64"""
    H, dk, R, L = 4, 16, 4, 9
    D = H * dk
    q, k, v, do, _ = A.make_inputs(profile, R, R, L, L, H, dk, seed=5)
    tok = torch.randint(1, 9, (R, L), generator=torch.Generator().manual_seed(2))
    tok[0] = A.PAD
    tok[1, 1:] = A.PAD
    tok[2, :-1] = A.PAD
    key_pad = tok.eq(A.PAD)
    mask = A.attn_mask(R, L, L, key_pad, causal)
    vid = torch.arange(R)
    ref = A.reference(q, k, v, do, vid, R, R, L, L, H, key_pad=key_pad, causal=causal)
    qd, kd, vd = [x.double().view(R, L, D).clone().requires_grad_(True) for x in (q, k, v)]
    o, p = _oracle_mha(qd, kd, vd, H, mask[:, 0])
    o.backward(do.double().view(R, L, D))
    assert torch.equal(ref["o"], o.detach().reshape(R * L, D)) and torch.equal(ref["p"], p.detach())
    for mine, theirs in ((ref["dq"], qd.grad), (ref["dk"], kd.grad), (ref["dv"], vd.grad)):
        assert float((mine - theirs.reshape(R * L, D)).abs().max()) < 1e-12
    # the all-<pad> sequence: P uniform over ALL keys, O the mean of V, dQ exactly 0, dK exactly 0 (its own memory here), dV = dO / L summed
    assert torch.equal(ref["p"][:, 0], torch.full((H, L, L), 1.0 / L, dtype=torch.float64))
    assert float((ref["o"][:L] - v[:L].double().mean(0, keepdim=True)).abs().max()) < 1e-15
    assert torch.equal(ref["dq"][:L], torch.zeros(L, D, dtype=torch.float64))
    assert torch.equal(ref["dk"][:L], torch.zeros(L, D, dtype=torch.float64))
    assert float((ref["dv"][:L] - do[:L].double().sum(0, keepdim=True) / L).abs().max()) < 1e-15
    if causal <= 1:
        # a partly masked row: no probability and no gradient at its filled keys
        assert float(ref["p"][:, 1, :, 1:].abs().max()) == 0.0 and float(ref["dk"][L + 1:2 * L].abs().max()) == 0.0
    else:
        # watch window 2 over a sequence whose only live key is the first: queries 2.. see nothing but <pad> -- filled rows arise
        # from key mask and window TOGETHER, and they too are uniform over all keys with no gradient to Q
        assert torch.equal(ref["p"][:, 1, 2:], torch.full((H, L - 2, L), 1.0 / L, dtype=torch.float64))
        assert torch.equal(ref["dq"][L + 2:2 * L], torch.zeros(L - 2, D, dtype=torch.float64))


def test_bf16_restatement_collapses_to_the_reference_without_rounding(monkeypatch):
    """the written-out backward of the restatement (rounding = identity) is autograd's; blocks of 64 keys with running statistics give
    the one-block forward"""
    H, dk, R, n_mem, Lq, Lk = 2, 16, 5, 2, 6, 150
    for profile in ("uniform", "rising", "sharp"):
        q, k, v, do, _ = A.make_inputs(profile, R, n_mem, Lq, Lk, H, dk, seed=1)
        vid, _, _ = A.row_map(R, "div", 2, n_mem)
        ref = A.reference(q, k, v, do, vid, n_mem, R, Lq, Lk, H)
        monkeypatch.setattr(A, "bf16_round", lambda x: x)
        res = A.reference(q, k, v, do, vid, n_mem, R, Lq, Lk, H, bf16=True, block=64)
        monkeypatch.undo()
        for name in ("o", "p", "dq", "dk", "dv"):
            scale = max(1.0, float(ref[name].abs().max()))
            assert float((ref[name] - res[name]).abs().max()) < 1e-12 * scale, (profile, name)


def test_row_maps_leave_the_last_memory_short():
    vid, kv_div, kv_mod = A.row_map(7, "div", 3, 3)
    assert vid.tolist() == [0, 0, 0, 1, 1, 1, 2] and (kv_div, kv_mod) == (3, 3)
    vid, kv_div, kv_mod = A.row_map(7, "mod", 1, 3)
    assert vid.tolist() == [0, 1, 2, 0, 1, 2, 0] and (kv_div, kv_mod) == (1, 3)
    vid, kv_div, kv_mod = A.row_map(11, "div", 2, 3)           # kv_mod wraps: sequences 6.. attend to memory 0 again
    assert vid.tolist() == [0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2]


@pytest.mark.parametrize("V,K", [(10547, 512), (101, 64)])
def test_duplicated_weight_rows_give_bit_equal_logits(V, K):
    g = torch.Generator().manual_seed(0)
    w, b, x = torch.randn(V, K, generator=g), torch.randn(V, generator=g), torch.randn(37, K, generator=g)
    pairs = [(3, 5), (17, V - 1), (V - 2, 64)]
    A.duplicate_rows(w, b, pairs)
    z = x @ w.t() + b
    for src, dst in pairs:
        assert torch.equal(z[:, src], z[:, dst])
