"""Inputs, the arithmetic model and the rounding bound for the direct tests of ts_attention_flash (attention_bf16_tiled_kernel,
theoremsearch_amd/csrc/kernels_attention_bf16_tiled.h): tests/test_attention_bf16_tiled_model_cpu.py and
tests/test_attention_bf16_tiled_gpu.py.  Plain torch on top of encoder_common and attention_bf16_common, no library: everything
here runs without a GPU.

Long selectors (selector_inputs).  attention_bf16_common.key_codes has 7 bits and serves 128 keys; here key k is the +-16 code of k's
12 bits, each bit repeated hd // 12 times (the remaining columns zero), for lengths up to 4,096.  Scores are integers below 2^24,
exact in fp32: 256 (hd // 12) (12 - 2 hamming(pi(i), k)).  Peak 15,360 / 30,720 / 64,512 for heads of 64 / 128 / 256, the best wrong
key 2,560 / 5,120 / 10,752 lower - further than zero_gap(hd) = 832 / 1,177 / 1,664, the distance at which exp2((s - m) scale log2e) is
exactly 0 in fp32.  Under the chunked online softmax: whatever the wrong keys of earlier chunks accumulated, when the picked key
arrives the rescale factor is exactly 0 and wipes it; in its chunk and every later one every other e is exactly 0 and l = 1, so the
row is V[pick] bit for bit.  Excluded keys hold 0x7F7F in K and V, picks are first / last / random, as in attention_bf16_common.

Model (emulate_online): the kernel's arithmetic per (query, chunk of `chunk` keys), in the kernel's order:
  fp32 scores; excluded keys replaced by a select; m_new = max(m, chunk max over the allowed keys); f = exp2((m - m_new) sl), exactly
  0 while m = -inf; e = exp2((s - m_new) sl) for the allowed keys, 0 otherwise; l = l f + sum e (unrounded e); P = bf16(e), to
  nearest even; o = o f + P V in fp32; at the end out = bf16(o (1 / l)), zeros where l = 0.  sl = fp32(scale) * fp32(log2 e).
`mutate` names one deliberate mistake (MUTANTS); the CPU test shows that the unmutated model passes every check of the GPU file and
that each mutant fails the checks CAUGHT_BY names.

Bound (bound), per element, from the fp64 reference on the same bf16 inputs (p, want in fp64, A = sum_k p_k |v_kd|):
    |got - want| <= 2^-8 (A + |want|) + n 2^-24 A
* 2^-8 A: P's rounding to bf16.  P is the UNNORMALISED e here, but the rounding is relative - at most 2^-8 (half a bf16 ulp) of every
  key's weight, whatever power of two the running maximum has scaled it by - and l sums the unrounded e;
* 2^-8 |want|: the output's rounding to bf16;
* n 2^-24 A: what fp32 leaves.  n counts the fp32 roundings on the path of ONE output element, from the kernel's own operation order:
    HD      the score: HD exact bf16 x bf16 products accumulated in fp32 through HD / 32 chained MFMAs;
    4       the exponent's argument and value: s - m_new, the product with sl, sl's own rounding, exp2;
    S       l: one fp32 addition per key (a lane's 4 C / 16 keys of a chunk in turn, the two shuffle additions, the addition into l);
    S       P V: one fp32 accumulation per key in the MFMA chain of the element's accumulator;
    6 per chunk, ceil(S / C) chunks: the factor f (m - m_new, the product with sl, exp2), l f, o f, and l f + sum e;
    2       1 / l and o (1 / l).
  n(HD, S, C) = HD + 4 + 2 S + 6 ceil(S / C) + 2.  Each rounding moves the element by at most 2^-24 of the weight that passes through
  it, and all weight is at most A.
None of it comes from what the kernel returns.
"""
import math

import torch

import attention_bf16_common as ab
import encoder_common as ec

CHUNK = {64: 128, 128: 64, 256: 32}                 # attn_bf16_tiled_chunk (encoder_plan.h; tests/attn_bf16_plan_check.cpp prints it)
SIGMA = {64: 1.5, 128: 1.2, 256: 1.0}               # the random inputs' scale
CODE_BITS, CODE_VALUE, CODE_KEYS = 12, 16.0, 4096
PICKS = ab.PICKS
HEADS = ((2, 2, 64), (4, 2, 128), (3, 1, 256))      # (query heads, key / value heads, head size) of the GPU file
WIDE_GROUP = (8, 1, 128)
LONG_LENGTHS = (1025, 2049)                         # B = 1, once per head shape
ONES_MIN_SEQ, ONES_MARGIN = ab.ONES_MIN_SEQ, ab.ONES_MARGIN
MASK_KINDS = ec.ATTN_MASK_KINDS + ("chunk_of_padding", "one_key")
MUTANTS = ("causal_lt", "drop_chunk_edge_key", "stale_buffer", "no_rescale_l", "masked_in_max", "neg_inf_nan", "truncate_p",
           "kv_head_mod", "causal_chunk_short", "other_scale")
# which checks of the GPU file reject each mutant (asserted by tests/test_attention_bf16_tiled_model_cpu.py on the GPU file's inputs)
CAUGHT_BY = {"causal_lt": ("selector", "bound"), "drop_chunk_edge_key": ("selector", "bound"), "stale_buffer": ("selector", "bound"),
             "no_rescale_l": ("bound",), "masked_in_max": ("selector",), "neg_inf_nan": ("selector", "bound"), "truncate_p": ("ones",),
             "kv_head_mod": ("selector", "bound"), "causal_chunk_short": ("selector", "bound"), "other_scale": ("bound",)}


def lengths(hd: int) -> tuple:
    """Every tile edge, query-block edge and chunk edge, and three or more chunks so that a buffer is reused."""
    C = CHUNK[hd]
    return tuple(sorted({1, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 17, 129, 257}))


def instantiation(hd: int, causal: bool) -> tuple:
    """(head size, causal) of attention_bf16_tiled_kernel that serves a call: encoder_ops.hip dispatches on exactly these two."""
    assert hd in CHUNK
    return (hd, bool(causal))


def all_instantiations() -> set:
    return {(hd, c) for hd in (64, 128, 256) for c in (False, True)}


def nchunk_of(hd: int, causal: bool, S: int, qblk: int) -> int:
    """The chunks the block of queries 64 qblk .. walks (the kernel's nchunk, re-stated)."""
    ct, T = CHUNK[hd] // 16, -(-S // 16)
    kt_blk = min(4 * qblk + 4, T) if causal else T
    return -(-kt_blk // ct)


def n_roundings(hd: int, S: int) -> int:
    return hd + 4 + 2 * S + 6 * (-(-S // CHUNK[hd])) + 2


# ---- small pieces --------------------------------------------------------------------------------------------------------------------
def scale_log2e(hd: int) -> float:
    """The host's fp32 constant: float(1 / sqrt(hd)) * float(log2 e), the product rounded to fp32."""
    return float(torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(ab.LOG2E, dtype=torch.float32))


def zero_gap(hd: int) -> int:
    """The smallest integer score distance d at which exp2(-d scale log2e) is exactly 0 in fp32: the argument is <= -150."""
    return math.ceil(150.0 / scale_log2e(hd))


def key_codes(hd: int) -> torch.Tensor:
    """[4096][hd] fp32: row k is the +-16 code of k's 12 bits, each repeated hd // 12 times, the remaining columns zero."""
    reps = hd // CODE_BITS
    bit = (torch.arange(CODE_KEYS)[:, None] >> torch.arange(CODE_BITS)[None, :]) & 1
    code = torch.zeros((CODE_KEYS, hd))
    code[:, :CODE_BITS * reps] = (bit.float() * 2.0 - 1.0).repeat_interleave(reps, dim=1) * CODE_VALUE
    return code


def selector_scores(hd: int) -> tuple:
    """(peak, gap) of the construction: a key's score against its own code, and the best wrong key's score minus that (< 0)."""
    reps = hd // CODE_BITS
    return CODE_VALUE ** 2 * reps * CODE_BITS, -2.0 * CODE_VALUE ** 2 * reps


def long_masks(B: int, S: int, hd: int, g: torch.Generator) -> dict:
    """The six kinds of ec.attention_masks and two more: left padding of C + 3 keys on every sequence (a whole chunk without an
    allowed key in front of every query), right padding that leaves key 0 alone."""
    out = dict(ec.attention_masks(B, S, g))
    ar = torch.arange(S)[None, :].expand(B, S)
    out["chunk_of_padding"] = (ar >= CHUNK[hd] + 3).to(torch.int64).contiguous()
    out["one_key"] = (ar == 0).to(torch.int64).contiguous()
    assert tuple(out) == MASK_KINDS
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_inputs(B: int, S: int, hq: int, hkv: int, hd: int):
    """qkv bf16 [B][S][(hq + 2 hkv) hd] ~ N(0, SIGMA[hd]^2) and one mask of each kind, seeded by the shape: the GPU file and the CPU
    file see the same ones."""
    g = ec._gen(17, B, S, hq, hkv, hd)
    qkv = (torch.randn((B, S, (hq + 2 * hkv) * hd), generator=g) * SIGMA[hd]).to(torch.bfloat16)
    return qkv, long_masks(B, S, hd, g)


def ones_inputs(B: int, S: int, hq: int, hkv: int, hd: int):
    """random_inputs with V = 1 everywhere: every output is the sum of the row's P over l."""
    qkv, masks = random_inputs(B, S, hq, hkv, hd)
    qkv.view(B, S, hq + 2 * hkv, hd)[:, :, hq + hkv:] = 1.0
    return qkv, masks


def selector_inputs(B: int, S: int, hq: int, hkv: int, hd: int, mask, causal: bool, pick: str, g: torch.Generator):
    """(qkv bf16 [B][S][(hq + 2 hkv) hd], pi int64 [B][S], has_key bool [B][S]) on the CPU: ab.selector_inputs with the 12-bit codes."""
    assert pick in PICKS and S <= CODE_KEYS and hq % hkv == 0
    allow = ab.allowed(mask, B, S, causal)
    has_key = allow.any(-1)
    ar = torch.arange(S)[None, None, :]
    if pick == "first":
        pi = torch.where(allow, ar, S).amin(-1)
    elif pick == "last":
        pi = torch.where(allow, ar, -1).amax(-1)
    else:
        pi = torch.where(allow, torch.rand((B, S, S), generator=g), -1.0).argmax(-1)
    pi = torch.where(has_key, pi, 0)
    code = key_codes(hd).to(torch.bfloat16)
    q = code[pi][:, :, None, :].expand(B, S, hq, hd)
    k = code[:S][None, :, None, :].expand(B, S, hkv, hd).contiguous()
    v = torch.randn((B, S, hkv, hd), generator=g).to(torch.bfloat16)
    if mask is not None:
        ab.fill_big(k, mask == 0)
        ab.fill_big(v, mask == 0)
    qkv = torch.cat((q, k, v), dim=2).reshape(B, S, (hq + 2 * hkv) * hd).contiguous()
    return qkv, pi, has_key


selector_want, pad_right, alone, bound_ratio, ones_share = ab.selector_want, ab.pad_right, ab.alone, ab.bound_ratio, ab.ones_share


# ---- the kernel's arithmetic -------------------------------------------------------------------------------------------------------------
def emulate_online(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, chunk: int, mutate=None) -> torch.Tensor:
    """bf16 [B][S][hq hd]: the module docstring's model, with the mistake `mutate` names (None: none):
    causal_lt: key < query for key <= query;  drop_chunk_edge_key: key C c of the last chunk c is left out;  stale_buffer: chunk
    c >= 2 multiplies chunk c - 2's V (a buffer overwritten too late);  no_rescale_l: o is rescaled, l is not;  masked_in_max: the
    running maximum takes the excluded keys' scores too;  neg_inf_nan: f is not forced to 0 at m = -inf;  truncate_p: P cut to bf16,
    not rounded;  kv_head_mod: query head h reads key / value head h % hkv;  causal_chunk_short: under causal a block of 64 queries
    stops one chunk early;  other_scale: another head size's 1 / sqrt(hd)."""
    assert mutate is None or mutate in MUTANTS, mutate
    B, S, _ = qkv.shape
    dev, f32 = qkv.device, torch.float32
    heads = torch.arange(hq, device=dev)
    kvh = heads % hkv if mutate == "kv_head_mod" else heads // (hq // hkv)
    x = qkv.view(B, S, hq + 2 * hkv, hd).float()
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv][:, :, kvh], x[:, :, hq + hkv:][:, :, kvh]
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k)
    allow = ab.allowed(mask, B, S, causal, dev, strict=mutate == "causal_lt")
    ar = torch.arange(S, device=dev)
    nch = -(-S // chunk)
    if mutate == "drop_chunk_edge_key":
        allow = allow & (ar != chunk * (nch - 1))[None, None, :]
    if mutate == "causal_chunk_short" and causal:
        ct, T = chunk // 16, -(-S // 16)
        walked = -(-torch.clamp(4 * (ar // 64) + 4, max=T) // ct) - 1                      # chunks a query's block still walks
        allow = allow & ((ar // chunk)[None, :] < walked[:, None])[None]
    allow = allow[:, None]                                                                   # [B][1][S][S]
    sl = scale_log2e({64: 128, 128: 64, 256: 128}[hd] if mutate == "other_scale" else hd)
    ninf, zero = torch.tensor(float("-inf"), dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev)
    m = torch.full((B, hq, S, 1), float("-inf"), dtype=f32, device=dev)
    l = torch.zeros((B, hq, S, 1), dtype=f32, device=dev)
    o = torch.zeros((B, hq, S, hd), dtype=f32, device=dev)
    for c in range(nch):
        lo, hi = c * chunk, min(S, (c + 1) * chunk)
        a, s = allow[..., lo:hi], sc[..., lo:hi]
        in_max = s if mutate == "masked_in_max" else torch.where(a, s, ninf)
        m_new = torch.maximum(m, in_max.amax(-1, keepdim=True))
        f = torch.exp2((m - m_new) * sl)
        if mutate != "neg_inf_nan":
            f = torch.where(m > ninf, f, zero)
        e = torch.where(a, torch.exp2((s - m_new) * sl), zero)
        l = (l if mutate == "no_rescale_l" else l * f) + e.sum(-1, keepdim=True)
        p = (e.view(torch.int32) & -65536).view(f32) if mutate == "truncate_p" else e.to(torch.bfloat16).float()
        vc = v[:, lo:hi]
        if mutate == "stale_buffer" and c >= 2:
            vc = v[:, lo - 2 * chunk:lo - 2 * chunk + (hi - lo)]
        o = o * f + torch.einsum("bhqk,bkhd->bhqd", p, vc)
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, zero)
    return (o * inv).permute(0, 2, 1, 3).to(torch.bfloat16).reshape(B, S, hq * hd)


# ---- the bound --------------------------------------------------------------------------------------------------------------------------------
def bound(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool):
    """(want fp64, has_key bool [B][S], bound fp64) [B][S][hq hd]: ec.attention_ref and the module docstring's bound; A is the same
    reference with |V| in V's place."""
    B, S, _ = qkv.shape
    scale = hd ** -0.5
    want, has_key = ec.attention_ref(qkv, mask, hq, hkv, hd, causal, scale)
    qa = qkv.clone()
    va = qa.view(B, S, hq + 2 * hkv, hd)[:, :, hq + hkv:]
    va.copy_(va.abs())
    A, _ = ec.attention_ref(qa, mask, hq, hkv, hd, causal, scale)
    u = ec.UNIT[torch.bfloat16]
    return want, has_key, u * (A + want.abs()) + n_roundings(hd, S) * ec.UNIT[torch.float32] * A
