"""Inputs, the arithmetic model and the rounding bound for the direct tests of the fp32 attention kernels behind ts_attention_float
(attention_f32_kernel, theoremsearch_amd/csrc/kernels_attention_f32.h) and ts_attention_tiled (attention_f32_tiled_kernel,
kernels_attention_tiled.h): tests/test_attention_f32_model_cpu.py and tests/test_attention_f32_gpu.py.  Plain torch on top of
encoder_common, attention_bf16_common and attention_bf16_tiled_common, no library: everything here runs without a GPU.

Selectors (selector_inputs).  Q and K are the +-16 twelve-bit codes of attention_bf16_tiled_common.key_codes, held as fp32; V is
full-mantissa fp32 random (not bf16-representable); every key the mask excludes holds 0x7F7F0000 (3.39e38) in K and in V.  Scores
are integers below 2^24: every product is +-256 or 0 and every partial sum an integer of at most 64,512, so the score is exact in
fp32 in ANY summation order - the MFMA's included.  The best wrong key lies 2,560 / 5,120 / 10,752 below the picked one, further
than zero_gap(hd) = 832 / 1,177 / 1,664, the distance at which exp2((s - m) scale log2e) is exactly 0 in fp32.  In the kernels'
running softmax over key tiles of 16: whatever the wrong keys of earlier tiles accumulated, when the picked key arrives the
rescale factor alpha is exactly 0 and wipes o and l; in that tile and every later one every other e is exactly 0, alpha is
exp2(0) = 1 and l = 1, so the row is 1.0 x V[pick] + 0 x finite = V[pick] bit for bit, and 1 / l = 1.  The excluded keys' scores
overflow to +-Inf or NaN (16 x 3.39e38 summed hd times) and are discarded by a select before anything reads them; their V rows are
multiplied by an exact 0.  A row without an allowed key keeps l = 0 and gives zeros.  With a projection bias that is zero on Q and
K and random on V (vbias_selector_inputs) the row is fp32(V[pick] + bias_v): the one rounding the kernels make while staging.

Model (emulate_f32): the kernels' arithmetic per (query, key tile of 16), in the kernels' order: fp32 scores; excluded scores
replaced by -inf through a select; m' = max(m, tile max); alpha = exp2((m - m') sl), or 1 while m' = -inf; e = exp2((s - m') sl)
for the allowed keys, 0 otherwise; l = l alpha + sum e; o = o alpha + e V; at the end o (1 / l), zeros where l = 0.
sl = fp32(scale) * fp32(log2 e).  The keys past S of the last tile are excluded and their V rows are zeros.  For `tiled`, the chunk
decides only which V rows a tile reads, so without a mutant the two entries are one computation.  `mutate` names one deliberate
mistake (MUTANTS); the CPU test shows that the unmutated model passes every check of the GPU file and that each mutant fails the
checks CAUGHT_BY names.

Bound.  Per element r = |got - want| / (2^-24 (A + |want|)), want and A = sum_k p_k |v_kd| from encoder_common.attention_ref in fp64
on the same fp32 inputs (unit()).  The limit per head size is LIMIT[hd] = 2 x the worst r of emulate_f32 (a plain torch fp32
evaluation of the kernels' sequence) over the GPU file's own random and ones-column inputs, the 1,025- and 2,049-token cases
included, rounded up.  The factor 2 is the project's convention (tests/test_encoder_ref_cpu.py keeps the same): it is what the
hardware's exp2 and the MFMA's unstated internal order get over torch's fp32.  The limit is measured against the model, never
against a kernel; tests/test_attention_f32_model_cpu.py recomputes the model's worst r and asserts
LIMIT / 2 >= worst r >= LIMIT / 4, so the table can neither be stale nor padded.
"""
import torch

import attention_bf16_common as ab
import attention_bf16_tiled_common as at
import encoder_common as ec

ENTRIES = ("float", "tiled")
KERNEL = {"float": "attention_f32_kernel", "tiled": "attention_f32_tiled_kernel"}
FLOAT_MAX_SEQ = {64: 512, 128: 256, 256: 128}       # attn_f32_max_seq (encoder_plan.h)
CHUNK = at.CHUNK                                    # attn_tiled_chunk (encoder_plan.h): 128 / 64 / 32 keys
BIG_BITS = 0x7F7F0000                               # 3.39e38: what every excluded key holds
SIGMA = at.SIGMA                                    # the random inputs' scale
B = 3
HEADS = ((4, 2, 64), (4, 2, 128), (4, 2, 256))      # 1 < hkv < hq at every head size: h // 2 and h % 2 differ at heads 1 and 2
WIDE_GROUP = (8, 1, 128)
LONG_LENGTHS = (1025, 2049)                         # tiled, B = 1, once per head shape
PICKS = at.PICKS
MASK_KINDS = at.MASK_KINDS
RANDOM_MASKS_LONG = "holes"

# LIMIT[hd] = 2 x the model's worst r, rounded up to the next multiple of 5 (the module docstring's bound).  MODEL_WORST: the model's
# worst r on the GPU file's inputs with torch 2.10 on a CPU, the same with 1 and with 8 threads - 40.40 at (4, 2, 64), 129 tokens,
# right padding; 35.40 at (4, 2, 128), 63 tokens, causal; 27.84 at (4, 2, 256), 113 tokens, holes; the ones column stays at 3 - 4.
# It does not grow with the length (the 2,049-token cases lie below it): what dominates is the score's own rounding, which the
# exponent multiplies by the score's size.  tests/test_attention_f32_model_cpu.py recomputes the figures and prints them next to
# this table.
MODEL_WORST = {64: 40.4, 128: 35.5, 256: 27.9}
LIMIT = {64: 85.0, 128: 75.0, 256: 60.0}

MUTANTS = ("causal_lt", "drop_last_key", "drop_chunk_edge_key", "stale_buffer", "causal_chunk_short", "no_rescale_l", "masked_in_max",
           "alpha_nan_at_neg_inf", "kv_head_mod", "other_scale", "vt_tail_not_zero", "v_bias_dropped", "k_bias_added_twice")
TILED_ONLY = ("drop_chunk_edge_key", "stale_buffer", "causal_chunk_short")        # mistakes in the staging of chunks
# which checks of the GPU file reject each mutant (asserted by tests/test_attention_f32_model_cpu.py on the GPU file's inputs):
# selector / vbias_selector - the two bit-for-bit families; bound - random inputs (with a projection bias) within LIMIT; ones - the
# ones column within LIMIT; poison - the selector after a launch that leaves +Inf in LDS (vt_tail_not_zero with finite leftovers
# changes nothing: 0 x finite = 0.  Only what the poisoning launch leaves makes it visible)
CAUGHT_BY = {"causal_lt": ("selector", "vbias_selector", "bound", "ones"), "drop_last_key": ("selector", "vbias_selector", "bound"),
             "drop_chunk_edge_key": ("selector", "vbias_selector", "bound"), "stale_buffer": ("selector", "vbias_selector", "bound"),
             "causal_chunk_short": ("selector", "vbias_selector", "bound"), "no_rescale_l": ("bound", "ones"),
             "masked_in_max": ("selector", "vbias_selector", "bound", "ones"), "alpha_nan_at_neg_inf": ("selector", "vbias_selector", "bound", "ones"),
             "kv_head_mod": ("selector", "vbias_selector", "bound"), "other_scale": ("bound",), "vt_tail_not_zero": ("poison",),
             "v_bias_dropped": ("vbias_selector", "bound"), "k_bias_added_twice": ("bound",)}
assert set(CAUGHT_BY) == set(MUTANTS)


# ---- the case list -------------------------------------------------------------------------------------------------------------------
def lengths(entry: str, hd: int) -> tuple:
    """tiled: every 16-token tile edge, 64-query block edge and chunk edge, three or more chunks (a buffer reused), 33 tokens (three
    waves of attention_f32_kernel), ts_attention_float's limit and one past it.  float: the same up to its limit - 1 / 2 / 3 / 4
    waves at 1 .. 16 / 17 / 33 / 63 .. tokens, and from 65 tokens on (T > 4) the causal rounds that start at the far end."""
    C, lim = CHUNK[hd], FLOAT_MAX_SEQ[hd]
    all_ = sorted({1, 15, 16, 17, 33, 63, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 17, 129, 257, lim, lim + 1})
    assert entry in ENTRIES
    return tuple(S for S in all_ if entry == "tiled" or S <= lim)


def float_waves(S: int) -> int:
    """Waves of attention_f32_kernel's workgroup at S tokens (attn_float_plan: 64 min(T, 4) threads)."""
    return min(-(-S // 16), 4)


def instantiation(entry: str, hd: int, causal: bool) -> tuple:
    """(kernel, head size, causal) that serves a call: encoder_ops.hip dispatches each entry on exactly these two values."""
    assert hd in CHUNK
    return (KERNEL[entry], hd, bool(causal))


def all_instantiations() -> set:
    return {(KERNEL[e], hd, c) for e in ENTRIES for hd in (64, 128, 256) for c in (False, True)}


def reached_instantiations() -> set:
    return {instantiation(e, hd, c) for e in ENTRIES for _, _, hd in HEADS + (WIDE_GROUP,) for c in (False, True)}


# ---- small pieces --------------------------------------------------------------------------------------------------------------------
scale_log2e, zero_gap, key_codes, selector_scores, long_masks = at.scale_log2e, at.zero_gap, at.key_codes, at.selector_scores, at.long_masks
allowed, selector_want, alone = ab.allowed, ab.selector_want, ab.alone


def big(device=None) -> torch.Tensor:
    return torch.tensor(BIG_BITS, dtype=torch.int32, device=device).view(torch.float32)


def fill_big(t: torch.Tensor, where: torch.Tensor) -> None:
    """Set the fp32 rows of `t` [B][S][...] that `where` [B][S] selects to 0x7F7F0000, in place."""
    t.view(torch.int32)[where.to(t.device)] = BIG_BITS


def pad_right(qkv: torch.Tensor, S: int):
    """ab.pad_right for fp32: the batch re-laid at length S, the extra tokens hold 0x7F7F0000 and the returned mask takes them out."""
    Bn, S0, w = qkv.shape
    out = torch.empty((Bn, S, w), dtype=qkv.dtype, device=qkv.device)
    out.view(torch.int32)[:] = BIG_BITS
    out[:, :S0] = qkv
    mask = (torch.arange(S, device=qkv.device)[None, :] < S0).to(torch.int64).expand(Bn, S).contiguous()
    return out, mask


def mask_out(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int) -> torch.Tensor:
    """K and V of every token the mask excludes set to 0x7F7F0000, in place (Q stays: an excluded token still asks)."""
    if mask is not None:
        Bn, S, _ = qkv.shape
        fill_big(qkv.view(Bn, S, hq + 2 * hkv, hd)[:, :, hq:], mask == 0)
    return qkv


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_inputs(Bn: int, S: int, hq: int, hkv: int, hd: int):
    """(qkv fp32 [Bn][S][(hq + 2 hkv) hd] ~ N(0, SIGMA[hd]^2), bias fp32 [(hq + 2 hkv) hd] ~ N(0, 0.5^2) over Q, K and V, masks of the
    eight kinds), seeded by the shape: the GPU file and the CPU file see the same ones.  masked(qkv, mask) is what a case runs on."""
    g = ec._gen(27, Bn, S, hq, hkv, hd)
    qkv = torch.randn((Bn, S, (hq + 2 * hkv) * hd), generator=g) * SIGMA[hd]
    bias = torch.randn(((hq + 2 * hkv) * hd,), generator=g) * 0.5
    return qkv, bias, long_masks(Bn, S, hd, g)


def ones_inputs(Bn: int, S: int, hq: int, hkv: int, hd: int):
    """random_inputs with V = 1 everywhere and no bias: every output is the row's sum of e over l."""
    qkv, _, masks = random_inputs(Bn, S, hq, hkv, hd)
    qkv.view(Bn, S, hq + 2 * hkv, hd)[:, :, hq + hkv:] = 1.0
    return qkv, masks


def masked(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, ones: bool = False) -> torch.Tensor:
    """A copy of the random / ones inputs for one mask: the excluded keys' K (and, for the random inputs, V) hold 0x7F7F0000, so a
    key that leaks with any weight at all, or a maximum taken over excluded scores, leaves the bound by dozens of orders."""
    out = mask_out(qkv.clone(), mask, hq, hkv, hd)
    if ones:
        Bn, S, _ = out.shape
        out.view(Bn, S, hq + 2 * hkv, hd)[:, :, hq + hkv:] = 1.0
    return out


def pick_keys(allow: torch.Tensor, pick: str, g: torch.Generator):
    """(pi int64 [B][S], has_key bool [B][S]): the first / last / a random allowed key of each query row; 0 for a row without one."""
    assert pick in PICKS
    Bn, S, _ = allow.shape
    has_key = allow.any(-1)
    ar = torch.arange(S)[None, None, :]
    if pick == "first":
        pi = torch.where(allow, ar, S).amin(-1)
    elif pick == "last":
        pi = torch.where(allow, ar, -1).amax(-1)
    else:
        pi = torch.where(allow, torch.rand((Bn, S, S), generator=g), -1.0).argmax(-1)
    return torch.where(has_key, pi, 0), has_key


def selector_inputs(Bn: int, S: int, hq: int, hkv: int, hd: int, mask, causal: bool, pick: str, g: torch.Generator):
    """(qkv fp32 [Bn][S][(hq + 2 hkv) hd], pi, has_key) on the CPU: the module docstring's construction.  V ~ N(0, 1) with its full
    fp32 mantissa, a different row for every (batch, key, key / value head)."""
    assert S <= at.CODE_KEYS and hq % hkv == 0
    pi, has_key = pick_keys(allowed(mask, Bn, S, causal), pick, g)
    code = key_codes(hd)
    q = code[pi][:, :, None, :].expand(Bn, S, hq, hd)
    k = code[:S][None, :, None, :].expand(Bn, S, hkv, hd)
    v = torch.randn((Bn, S, hkv, hd), generator=g)
    qkv = torch.cat((q, k, v), dim=2).reshape(Bn, S, (hq + 2 * hkv) * hd).contiguous()
    return mask_out(qkv, mask, hq, hkv, hd), pi, has_key


def vbias_selector_inputs(Bn: int, S: int, hq: int, hkv: int, hd: int, mask, causal: bool, pick: str, g: torch.Generator):
    """(qkv, bias, pi, has_key): selector_inputs and a projection bias that is zero on Q and K and ~ N(0, 1) on V."""
    qkv, pi, has_key = selector_inputs(Bn, S, hq, hkv, hd, mask, causal, pick, g)
    bias = torch.zeros(((hq + 2 * hkv), hd))
    bias[hq + hkv:] = torch.randn((hkv, hd), generator=g)
    return qkv, bias.reshape(-1).contiguous(), pi, has_key


def vbias_selector_want(qkv: torch.Tensor, bias: torch.Tensor, pi, has_key, hq: int, hkv: int, hd: int) -> torch.Tensor:
    """fp32(V[pick] + bias_v), zeros in the rows without a key."""
    Bn, S, w = qkv.shape
    full = qkv.clone()
    full.view(Bn, S, hq + 2 * hkv, hd)[:, :, hq + hkv:] += bias.to(qkv.device).view(hq + 2 * hkv, hd)[hq + hkv:]
    return selector_want(full, pi, has_key, hq, hkv, hd)


def selector_case(hq: int, hkv: int, hd: int, S: int, kind: str, causal: bool, pick: str, vbias: bool = False):
    """(qkv, bias or None, mask, has_key, want) of one selector case at B = 3, on the CPU, seeded by the case: the CPU file and the
    GPU file run the same ones."""
    mask = long_masks(B, S, hd, ec._gen(28, S, hd))[kind]
    g = ec._gen(29, hq, hkv, hd, S, MASK_KINDS.index(kind), int(causal), PICKS.index(pick), int(vbias))
    if vbias:
        qkv, bias, pi, has_key = vbias_selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, g)
        return qkv, bias, mask, has_key, vbias_selector_want(qkv, bias, pi, has_key, hq, hkv, hd)
    qkv, pi, has_key = selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, g)
    return qkv, None, mask, has_key, selector_want(qkv, pi, has_key, hq, hkv, hd)


def bound_cases(entry: str, hq: int, hkv: int, hd: int):
    """(Bn, S, kind) of the random and ones-column sweeps: B = 3 at every length of the entry under every mask kind, and for `tiled`
    one sequence of 1,025 and of 2,049 tokens with holes."""
    for S in lengths(entry, hd):
        for kind in MASK_KINDS:
            yield B, S, kind
    if entry == "tiled":
        for S in LONG_LENGTHS:
            yield 1, S, RANDOM_MASKS_LONG


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------------------------
def emulate_f32(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, entry: str, mutate=None, *, bias=None,
                tail: float = 1.0) -> torch.Tensor:
    """fp32 [B][S][hq hd]: the module docstring's model, with the mistake `mutate` names (None: none):
    causal_lt: key < query for key <= query;  drop_last_key: the last allowed key of each row is left out;  drop_chunk_edge_key:
    key C c of the last chunk c is left out;  stale_buffer: chunk c >= 2 reads chunk c - 2's V (a buffer overwritten too late);
    causal_chunk_short: under causal a block of 64 queries stops one chunk early;  no_rescale_l: o is rescaled, l is not;
    masked_in_max: the running maximum takes the excluded keys' scores too;  alpha_nan_at_neg_inf: alpha is not forced to 1 while
    m' = -inf;  kv_head_mod: query head h reads key / value head h % hkv;  other_scale: another head size's 1 / sqrt(hd);
    vt_tail_not_zero: the keys >= S of the last tile read V = `tail`, not zeros;  v_bias_dropped: V without its share of the bias;
    k_bias_added_twice: K's share of the bias is added on every tile into fragments the reload does not reset - tile j sees
    K + (j + 1) bias_k.  The three mistakes in the staging of chunks exist for `tiled` only."""
    assert entry in ENTRIES and (mutate is None or mutate in MUTANTS), (entry, mutate)
    assert not (entry == "float" and mutate in TILED_ONLY), (entry, mutate)
    Bn, S, _ = qkv.shape
    assert entry == "tiled" or S <= FLOAT_MAX_SEQ[hd]
    dev, f32 = qkv.device, torch.float32
    assert qkv.dtype == f32
    heads = torch.arange(hq, device=dev)
    kvh = heads % hkv if mutate == "kv_head_mod" else heads // (hq // hkv)
    x = qkv.view(Bn, S, hq + 2 * hkv, hd)
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv], x[:, :, hq + hkv:]
    kb = None
    if bias is not None:
        bb = bias.to(dev).view(hq + 2 * hkv, hd)
        q, kb = q + bb[:hq], bb[hq:hq + hkv][kvh]
        if mutate != "v_bias_dropped":
            v = v + bb[hq + hkv:]
    k, v = k[:, :, kvh], v[:, :, kvh]
    T = -(-S // 16)
    SP = 16 * T
    if SP > S:                                                                              # the last tile's keys past S
        k = torch.cat((k, k[:, S - 1:S].expand(Bn, SP - S, hq, hd)), dim=1)                 # (the kernels clamp the row; excluded below)
        v = torch.cat((v, torch.full((Bn, SP - S, hq, hd), tail if mutate == "vt_tail_not_zero" else 0.0, dtype=f32, device=dev)), dim=1)
    allow = allowed(mask, Bn, S, causal, dev, strict=mutate == "causal_lt")
    ar = torch.arange(S, device=dev)
    if mutate == "drop_last_key":
        allow = allow & (ar[None, None, :] != torch.where(allow, ar[None, None, :], -1).amax(-1, keepdim=True))
    C = CHUNK[hd]
    if mutate == "drop_chunk_edge_key":
        allow = allow & (ar != C * ((S - 1) // C))[None, None, :]
    if mutate == "causal_chunk_short" and causal:
        walked = -(-torch.clamp(4 * (ar // 64) + 4, max=T) // (C // 16)) - 1                # chunks a query's block still walks
        allow = allow & ((ar // C)[None, :] < walked[:, None])[None]
    allow = torch.nn.functional.pad(allow, (0, SP - S))[:, None]                            # [B][1][S][SP]
    sl = torch.tensor(scale_log2e({64: 128, 128: 64, 256: 128}[hd] if mutate == "other_scale" else hd), dtype=f32, device=dev)
    ninf, zero, one = (torch.tensor(c, dtype=f32, device=dev) for c in (float("-inf"), 0.0, 1.0))
    in_seq = (torch.arange(SP, device=dev) < S)
    m = torch.full((Bn, hq, S, 1), float("-inf"), dtype=f32, device=dev)
    l = torch.zeros((Bn, hq, S, 1), dtype=f32, device=dev)
    o = torch.zeros((Bn, hq, S, hd), dtype=f32, device=dev)
    for kj in range(T):
        lo, hi = 16 * kj, 16 * kj + 16
        kt = k[:, lo:hi]
        if kb is not None:
            for _ in range(kj + 1 if mutate == "k_bias_added_twice" else 1):
                kt = kt + kb
        s = torch.einsum("bqhd,bkhd->bhqk", q, kt)
        a = allow[..., lo:hi]
        in_max = torch.where(in_seq[lo:hi], s, ninf) if mutate == "masked_in_max" else torch.where(a, s, ninf)
        m_new = torch.maximum(m, in_max.amax(-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * sl)
        if mutate != "alpha_nan_at_neg_inf":
            alpha = torch.where(m_new > ninf, alpha, one)
        e = torch.where(a, torch.exp2((s - m_new) * sl), zero)
        l = (l if mutate == "no_rescale_l" else l * alpha) + e.sum(-1, keepdim=True)
        vlo = lo
        if mutate == "stale_buffer" and lo // C >= 2:
            vlo = lo - 2 * C
        o = o * alpha + torch.einsum("bhqk,bkhd->bhqd", e, v[:, vlo:vlo + 16])
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, zero)
    return (o * inv).permute(0, 2, 1, 3).reshape(Bn, S, hq * hd).contiguous()


# ---- the bound --------------------------------------------------------------------------------------------------------------------------------
def unit(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, bias=None, ones: bool = False):
    """(want fp64, has_key bool [B][S], 2^-24 (A + |want|) fp64) [B][S][hq hd]: ec.attention_ref; A is the same reference with |V| in V's
    place.  `ones`: V = 1, so want = A = 1 in every row with a key, without the arithmetic."""
    Bn, S, _ = qkv.shape
    scale = hd ** -0.5
    if ones:
        has_key = allowed(mask, Bn, S, causal, qkv.device).any(-1)
        want = has_key[:, :, None].expand(Bn, S, hq * hd).double()
        return want, has_key, ec.UNIT[torch.float32] * 2.0 * want
    want, has_key = ec.attention_ref(qkv, mask, hq, hkv, hd, causal, scale, bias=bias)
    qa = (qkv if bias is None else qkv + bias.to(qkv.device)).clone()
    va = qa.view(Bn, S, hq + 2 * hkv, hd)[:, :, hq + hkv:]
    va.copy_(va.abs())
    A, _ = ec.attention_ref(qa, mask, hq, hkv, hd, causal, scale)
    return want, has_key, ec.UNIT[torch.float32] * (A + want.abs())


def worst_r(got: torch.Tensor, want: torch.Tensor, has_key: torch.Tensor, u: torch.Tensor) -> float:
    """The worst r = |got - want| / unit over the rows with a key; 1e30 where the error is not finite or a zero unit is missed."""
    return ab.bound_ratio(got, want, has_key, u)
