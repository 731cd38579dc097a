"""Shared by tests/test_attention_edges_gpu.py (GPU) and tests/test_attention_refs_cpu.py (CPU): the float64 reference of the
attention core, the generator of score profiles that uniform random inputs never reach, and the error bars that follow from them.
Nothing here touches the GPU, so generator and reference are themselves checked without one.

Score profiles.  Scores are s[q, key] = Q[q] . K[key] / sqrt(dk) per head.  The structure sits in a few reserved coordinates of
every head (uniform noise of amplitude `noise` fills the rest), so it is known by construction and the reference needs nothing
special:
  coordinate 0          Q = C_BASE for every query, K[key] = base[key] * sqrt(dk) / C_BASE: adds base[key] to every query's scores;
  coordinate 1 + t      one-hot: queries whose winner is the t-th entry of `winners` hold C_WIN there, that key holds
                        SHARP * sqrt(dk) / C_WIN: adds SHARP to exactly one key of such a query (the winner differs per query).
                        `sharp` (+30) drives P to 1 and dS to about 1e-9; `peaked` (+5) leaves the winner about half of the mass.
"""
import math

import torch

PAD = 0
C_BASE = 4.0         # exact in bf16
C_WIN = 2.0
SHARP = 30.0
PEAK = 5.0           # a winner that takes about half of the mass: dS = P (dP - delta) at P neither 0 nor 1
PROFILES = ("uniform", "sharp", "peaked", "rising", "falling", "all_low", "all_high", "twin")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def winner_keys(Lk, dk):
    """keys a sharp query may single out: first / last key, both sides of the first 16-key tile edge, of every wave's key quarter
    (32) and of every streaming block (64); at most dk - 5 of them (coordinates are few at dk = 16)"""
    cand = [0, Lk - 1, 15, 16, 31, 32, 63, 64, 95, 96, 127, 128, 191, 192, 255, 256]
    keys = []
    for k in cand:
        if 0 <= k < Lk and k not in keys:
            keys.append(k)
    return keys[:dk - 5]


def base_profile(profile, Lk, seed=0):
    """the part of the scores shared by all queries, [Lk] float64 (before the +-1.3 of the noise coordinates)"""
    key = torch.arange(Lk, dtype=torch.float64)
    if profile in ("uniform", "sharp", "peaked", "twin"):
        return torch.zeros(Lk, dtype=torch.float64)
    if profile == "rising":          # +11 per 16-key tile: the maximum rises by 22 per wave share of 32 keys, 44 per 64-key block
        return 11.0 * torch.floor(key / 16)
    if profile == "falling":         # the maximum in the first tile, everything after it 115 below: exp underflows to exactly 0
        return torch.where(key < 16, torch.zeros_like(key), torch.full_like(key, -115.0))
    u = rnd(Lk, seed=seed + 77).double()
    if profile == "all_low":         # [-93, -82] + noise: every score in [-95, -80]
        return -87.5 + 5.5 * u
    if profile == "all_high":
        return 87.5 + 5.5 * u
    raise ValueError(profile)


def twin_keys(Lk):
    """two keys that share one bit-identical K row: in different 64-key blocks / wave quarters where the memory has them"""
    if Lk < 2:
        return None
    if Lk > 96:
        return (31, Lk - 1) if Lk <= 128 else (31, 64 * ((Lk - 1) // 64))
    return (0, Lk - 1)


def make_inputs(profile, R, n_mem, Lq, Lk, H, dk, seed=0, noise=1.0):
    """q [R * Lq, D], k / v [n_mem * Lk, D], do [R * Lq, D] in float32 with the profile planted per head, and `info`:
    winners [R, Lq] (key index or -1), base [Lk], twins"""
    D = H * dk
    sq = math.sqrt(dk)
    q, k = rnd(R * Lq, D, seed=seed + 1, scale=noise), rnd(n_mem * Lk, D, seed=seed + 2, scale=noise)
    v, do = rnd(n_mem * Lk, D, seed=seed + 3), rnd(R * Lq, D, seed=seed + 4)
    info = {"winners": torch.full((R, Lq), -1, dtype=torch.long), "base": base_profile(profile, Lk, seed), "twins": None}
    if profile == "uniform":
        return q, k, v, do, info
    wk = winner_keys(Lk, dk) if profile in ("sharp", "peaked") else []
    gap = SHARP if profile == "sharp" else PEAK
    n_res = 1 + len(wk)
    qv, kv = q.view(R, Lq, H, dk), k.view(n_mem, Lk, H, dk)
    qv[..., :n_res] = 0.0
    kv[..., :n_res] = 0.0
    qv[..., 0] = C_BASE
    kv[..., 0] = (info["base"] * sq / C_BASE).float().view(1, Lk, 1)
    for t, key in enumerate(wk):
        kv[:, key, :, 1 + t] = gap * sq / C_WIN
    if wk:
        for r in range(R):
            for i in range(Lq):
                t = (i + r) % len(wk)
                qv[r, i, :, 1 + t] = C_WIN
                info["winners"][r, i] = wk[t]
    if profile == "twin":
        tw = twin_keys(Lk)
        if tw is not None:
            a, b = tw
            kv[:, a, :, 0] = 25.0 * sq / C_BASE
            kv[:, b] = kv[:, a]                  # the whole row, noise included: the two scores are the same bits
            info["twins"] = tw
            info["base"][a] = info["base"][b] = 25.0
    return q, k, v, do, info


def row_map(R, mode, k_, n_mem):
    """sequence -> memory, as the C ABI's (kv_div, kv_mod): "mod" r % n_mem (the passes of a training step), "div" (r // k_) % n_mem
    (the candidates of a length beam); R need not be a multiple of k_ * n_mem"""
    r = torch.arange(R)
    if mode == "mod":
        return r % n_mem, 1, n_mem
    return (r // k_) % n_mem, k_, n_mem


def attn_mask(R, Lq, Lk, key_pad=None, causal=0):
    """bool [R, 1, Lq, Lk], True = filled with -10e6.  key_pad [R, Lk]; causal = 1: keys after the query; causal = 1 + w: also the
    keys k <= q - w (--watch w: a query sees itself and the w - 1 tokens before it)"""
    m = torch.zeros(R, 1, Lq, Lk, dtype=torch.bool)
    if key_pad is not None:
        m = m | key_pad.view(R, 1, 1, Lk)
    if causal:
        qi, ki = torch.arange(Lq).view(Lq, 1), torch.arange(Lk).view(1, Lk)
        c = ki > qi
        if causal > 1:
            c = c | (ki <= qi - (causal - 1))
        m = m | c.view(1, 1, Lq, Lk)
    return m


def heads(x, H):
    R, L, D = x.shape
    return x.view(R, L, H, D // H).permute(0, 2, 1, 3)


def mha_ref(q, k, v, H, key_pad=None, causal=0, rounding=None, block=None):
    """softmax(masked_fill(Q K^T / sqrt(dk), mask, -10e6)) V per head, in the dtype of its inputs (float64 in the tests).
    q [R, Lq, D], k / v [R, Lk, D] (gathered per sequence).  Returns o [R, Lq, D], p [H, R, Lq, Lk].  Differentiable: the
    gradients of the tests come from autograd, where masked_fill passes nothing to a filled position.
    rounding: None, or a function applied to every matrix-instruction operand (the bf16-operand kernels); with `block` the forward
    runs as the streaming kernel does: unnormalised exp(S - running maximum) is the rounded operand per block of `block` keys."""
    R, Lq, D = q.shape
    Lk = k.shape[1]
    dk = D // H
    rd = rounding if rounding is not None else (lambda x: x)
    qh, kh, vh = heads(q, H), heads(k, H), heads(v, H)
    s = rd(qh) @ rd(kh).transpose(-1, -2) / math.sqrt(dk)
    s = s.masked_fill(attn_mask(R, Lq, Lk, key_pad, causal), -10e6)
    p = torch.softmax(s, -1)
    if block is None:
        o = rd(p) @ rd(vh)
    else:
        m = torch.full(s.shape[:-1] + (1,), -float("inf"), dtype=s.dtype)
        acc = torch.zeros(R, H, Lq, dk, dtype=s.dtype)
        for k0 in range(0, Lk, block):
            sb = s[..., k0:k0 + block]
            m_new = torch.maximum(m, sb.max(-1, keepdim=True).values)
            acc = acc * torch.exp(m - m_new) + rd(torch.exp(sb - m_new)) @ rd(vh[:, :, k0:k0 + block])
            m = m_new
        o = acc / torch.exp(s - m).sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(R, Lq, D), p.permute(1, 0, 2, 3)


def bf16_round(x):
    return x.float().to(torch.bfloat16).to(x.dtype)


def reference(q, k, v, do, vid, n_mem, R, Lq, Lk, H, key_pad=None, causal=0, bf16=False, block=None):
    """float64 results of one case from float32 inputs laid out as the C ABI takes them: o [R*Lq, D], p [H, R, Lq, Lk],
    dq [R*Lq, D], dk / dv [n_mem*Lk, D] (summed over the sequences of a memory), and `aux`, what the error bars need.
    bf16: the rounding restatement of the bf16-operand kernels (operands of every contraction rounded, soft-max in full precision),
    gradients written out, not autograd: P and dS are rounded operands of the backward contractions."""
    D = q.shape[1]
    dk = D // H
    sq = math.sqrt(dk)
    qd = q.double().view(R, Lq, D).clone().requires_grad_(True)
    kd = k.double().view(n_mem, Lk, D).clone().requires_grad_(True)
    vd = v.double().view(n_mem, Lk, D).clone().requires_grad_(True)
    dod = do.double().view(R, Lq, D)
    mask = attn_mask(R, Lq, Lk, key_pad, causal)
    with torch.no_grad():
        kk, vv = kd[vid], vd[vid]
        qh, kh, vh, doh = heads(qd, H), heads(kk, H), heads(vv, H), heads(dod, H)
    if not bf16:
        o, p = mha_ref(qd, kd[vid], vd[vid], H, key_pad, causal)
        o.backward(dod)
        res = {"o": o.detach().reshape(R * Lq, D), "p": p.detach(), "dq": qd.grad.reshape(R * Lq, D),
               "dk": kd.grad.reshape(n_mem * Lk, D), "dv": vd.grad.reshape(n_mem * Lk, D)}
        rd = lambda x: x
    else:
        rd = bf16_round
    with torch.no_grad():
        if bf16:
            o, p = mha_ref(qd, kk, vv, H, key_pad, causal, rounding=rd, block=block)
        ph = p.detach().permute(1, 0, 2, 3)
        dp = rd(doh) @ rd(vh).transpose(-1, -2)
        centred = dp - (ph * dp).sum(-1, keepdim=True)
        # masked_fill passes no gradient: dS is 0 at filled positions (already 0 through P unless the whole row is filled)
        ds = (ph * centred / sq).masked_fill(mask, 0.0)
        back = lambda x, L: x.permute(0, 2, 1, 3).reshape(R, L, D)
        if bf16:
            dk_seq = back(rd(ds).transpose(-1, -2) @ rd(qh), Lk)
            dv_seq = back(rd(ph).transpose(-1, -2) @ rd(doh), Lk)
            res = {"o": o.reshape(R * Lq, D), "p": p, "dq": back(rd(ds) @ rd(kh), Lq).reshape(R * Lq, D),
                   "dk": torch.zeros(n_mem, Lk, D, dtype=torch.float64).index_add_(0, vid, dk_seq).reshape(n_mem * Lk, D),
                   "dv": torch.zeros(n_mem, Lk, D, dtype=torch.float64).index_add_(0, vid, dv_seq).reshape(n_mem * Lk, D)}
        res["aux"] = {
            "P": ph, "dS": ds.abs(), "Q": rd(qh).abs(), "K": rd(kh).abs(), "V": rd(vh).abs(), "dO": rd(doh).abs(), "vid": vid,
            "n_mem": n_mem, "sq": sq, "dk": dk,
            # bound of the fp32 dot product's rounding error: |fl(q.k) - q.k| <= gamma * sum_d |q_d k_d|
            "S": float(((qh.abs() @ kh.abs().transpose(-1, -2)) / sq).masked_fill(mask, 0.0).max()),
            # per query row: the larger of max_k |dP - delta| and max_k |dP| over its live keys
            "G": torch.maximum(centred.abs(), dp.abs()).masked_fill(mask, 0.0).max(-1, keepdim=True).values,
        }
    return res


def bars(ref, profile, bf16=False, long_rows=False, n_terms=2):
    """Error bars PER ELEMENT of every output (tensors shaped like the outputs), derived, not tuned: the bar the suite already
    holds on uniform inputs plus a bound of what the profile adds, propagated through |P|, |dS|, |Q|, |K|, |V|, |dO| of the
    reference.  A planted coordinate (|K| of several hundred in ONE of dk columns) widens the bar of its own column only.

    fp32 operands.  The fp32 score carries an absolute error of about eps_s = 4 * 2^-24 * S (S: the largest sum_d |q_d k_d| / sqrt(dk);
    4 for the accumulation, the division and expf's argument), which is a RELATIVE error rel = 2 eps_s in P (numerator and sum).
    dP = dO V^T carries e_dp = dk * 2^-24 (|dO|, |V| <= 1).  With dS = P (dP - delta) / sqrt(dk):
      |err dS| <= P (2 rel G + 2 e_dp) / sqrt(dk) + 2^-22 |dS|          G: the row's max of |dP - delta| and |dP|
      O   base + rel (P @ |V|)            P   1e-5 + rel P
      dQ  5e-5 + |err dS| @ |K|           dK  base + sum over the memory's sequences of |err dS|^T @ |Q|
      dV  base + the same sum of (rel P)^T @ |dO|
    base: O 2e-5 (5e-5 over 100+ keys); dK / dV 5e-5 (1e-4 over 100+ keys, 2e-4 with more than two sequences per memory).
    On `uniform` every addition is dropped: exactly today's bars.

    bf16 operands (against the rounding restatement; bases as in the existing tests: O 1e-3, dQ 2e-3, dK / dV 4e-3).  The kernel's
    fp32 soft-max and the restatement's float64 one differ by rel, which moves an operand that sits on a bf16 rounding boundary by
    one step: up to 2^-7 relative (8 significant bits).  Every P and dS element is allowed that step on top of the fp32 terms above."""
    a = ref["aux"]
    P, dS, sq, vid, n_mem = a["P"], a["dS"], a["sq"], a["vid"], a["n_mem"]
    R, H, Lq, Lk = P.shape
    D = H * a["dk"]
    plain = profile == "uniform"
    rel = 0.0 if plain else 2 * 4 * 2.0 ** -24 * a["S"]
    e_dp = 0.0 if plain else a["dk"] * 2.0 ** -24
    step = 2.0 ** -7 if (bf16 and not plain) else 0.0
    gam = 0.0 if plain else 2.0 ** -22
    ds_err = P * (2 * rel * a["G"] + 2 * e_dp) / sq + (gam + step) * dS
    p_err = (rel + step) * P
    back = lambda x, L: x.permute(0, 2, 1, 3).reshape(R, L, D)
    per_mem = lambda x: torch.zeros(n_mem, Lk, D, dtype=torch.float64).index_add_(0, vid, x).reshape(n_mem * Lk, D)
    if bf16:
        base = {"o": 1e-3, "dq": 2e-3, "dk": 4e-3, "dv": 4e-3}
    else:
        base_kv = 2e-4 if n_terms > 2 else (1e-4 if long_rows else 5e-5)
        base = {"o": 5e-5 if long_rows else 2e-5, "dq": 5e-5, "dk": base_kv, "dv": base_kv}
    return {"o": base["o"] + back(p_err @ a["V"], Lq).reshape(R * Lq, D),
            "p": 1e-5 + (rel * P).permute(1, 0, 2, 3),
            "dq": base["dq"] + back(ds_err @ a["K"], Lq).reshape(R * Lq, D),
            "dk": base["dk"] + per_mem(back(ds_err.transpose(-1, -2) @ a["Q"], Lk)),
            "dv": base["dv"] + per_mem(back((p_err + gam * P).transpose(-1, -2) @ a["dO"], Lk))}


def duplicate_rows(w, bias, pairs):
    """in place: weight row (and bias) `dst` becomes a copy of `src` for every (src, dst) -- the logits of the two columns are then
    the same bits in any GEMM that accumulates every output column over K in the same order"""
    for src, dst in pairs:
        w[dst] = w[src]
        if bias is not None:
            bias[dst] = bias[src]
    return w, bias
