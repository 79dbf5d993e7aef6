"""Inputs, the arithmetic model and the rounding bound for the direct tests of the bf16 attention kernels behind
ts_attention_short and ts_attention_gqa (tests/test_attention_bf16_model_cpu.py, tests/test_attention_bf16_gpu.py).  Plain torch on
top of encoder_common (attention_masks, attention_ref, guarded, assert_margins, UNIT), no library: everything here runs without
a GPU.  ts_attention_short's layout [B][S][3][H][64] is the stacked layout [B][S][(hq + 2 hkv) hd] with hq = hkv = H, so one
reference and one model serve both entries.

Selectors (selector_inputs): inputs whose softmax is exactly one-hot in the kernels' own arithmetic.  Key k is the +-8 code of k's 7
bits, each bit repeated hd // 7 times (the remaining columns zero), the same in every key / value head; query row i is the code of
a chosen allowed key pi(i).  Scores are integers below 2^24, exact in fp32: 64 (hd // 7) (7 - 2 hamming(pi(i), k)).  The closest
wrong key lies selector_scores(hd)[1] lower, further than zero_gap(hd), the distance at which exp2f((s - m) scale log2e) is exactly
0 in fp32 (its argument is <= -150: 2^-150 is the tie between 0 and the smallest denormal and rounds to even).  So e = 1 at pi(i)
and 0 elsewhere, the sum is 1, P is 1.0 / 0.0, and the row's output is V[b, pi(i), kv head] bit for bit.  The K rows and V rows of
the keys the mask excludes hold 0x7F7F, the largest finite bf16: an excluded key's score is discarded and 0 x finite is 0, so a key
that leaks turns the row into Inf / NaN or something huge.  The peak score 64 (hd // 7) 7 overflows exp2f without the max subtraction.

Model (emulate): fp32 scores, max subtraction, exp2 with the kernels' fp32 scale constant, normalise, P to bf16 round-to-nearest-
even, fp32 P V, out to bf16; a keyless row gives zeros.  `mutate` names one deliberate mistake (MUTANTS); the CPU test shows that
the unmutated model passes every check of the GPU file and that each mutant fails the checks CAUGHT_BY names.

Bound (bound), per element, from the fp64 reference on the same bf16 inputs (p, want in fp64, A = sum_k p_k |v_kd|):
    |got - want| <= 2^-8 (A + |want|) + 2^-16 A
* 2^-8 A: P's rounding to bf16 - a relative error of at most 2^-8 (half a bf16 ulp) on every key's weight;
* 2^-8 |want|: the output's rounding to bf16;
* 2^-16 A: what fp32 leaves - the score's 64- / 128-term sum and exp2f's argument (a relative error of the weight of about
  |s - m| scale log2e 2^-24 <= 2^-18 at the |s - m| < 64 that still carries weight), exp2f and the reciprocal (a few ulps), the S-term
  sums of the weights and of P V: all of order (hd + S) 2^-24 <= 2^-16 of A.
None of it comes from what the kernels return.
"""
import math

import torch

import encoder_common as ec

BIG_BITS = 0x7F7F                                   # the largest finite bf16 (3.39e38)
HEAD_DIM = {"short": 64, "gqa": 128}
SIGMA = {64: 1.5, 128: 1.2}                         # the random inputs' scale, as tests/test_mirrors_gpu.py has them
LOG2E = 1.4426950408889634
CODE_BITS, CODE_VALUE = 7, 8.0
PICKS = ("first", "last", "random")
MUTANTS = ("causal_lt", "drop_last_key", "drop_tile_edge_key", "other_scale", "truncate_p", "kv_head_mod", "swap_key_pair",
           "stale_pad", "no_max")
# which checks of the GPU file reject each mutant (asserted by tests/test_attention_bf16_model_cpu.py on the GPU file's inputs)
CAUGHT_BY = {"causal_lt": ("selector", "bound"), "drop_last_key": ("selector", "bound"), "drop_tile_edge_key": ("selector", "bound"),
             "other_scale": ("bound",), "truncate_p": ("bound", "ones"), "kv_head_mod": ("selector", "bound"),
             "swap_key_pair": ("selector", "bound"), "stale_pad": ("selector", "bound"), "no_max": ("selector",)}

# every T = 1 .. 8 with a full tile, one token short of it and one over; the odd T take the zero-filled V^T / P columns
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128)
ODD_TILE_LENGTHS = tuple(S for S in LENGTHS if -(-S // 16) % 2 == 1)
SHORT_HEADS = (1, 5, 12)                            # B H = 3, 15: idle waves in the last workgroup; 12: the real head stride
GQA_HEADS = ((1, 1), (3, 1), (4, 2), (6, 2), (8, 1), (16, 8))
ONES_MIN_SEQ = 64                                   # the ones-column share is asserted from this length on
ONES_MARGIN = 0.25                                  # ... as the model's own share minus this (the CPU test: truncation still fails)


# ---- the launch rules of encoder_plan.h (attn_short_plan, attn_gqa_plan), re-stated --------------------------------------------------
def kernel_of(entry: str, S: int, hq: int = 1, hkv: int = 1, causal: bool = False) -> tuple:
    """(kernel, T, causal, R) a call is served by; causal / R are None where the kernel has no such parameter."""
    T = -(-S // 16)
    assert 1 <= S <= 128
    if entry == "short":
        return ("attention_rows_kernel" if S > 64 else "attention_short_kernel", T, None, None)
    if S <= 64:
        return ("attention_gqa_kernel", T, bool(causal), None)
    per_kv = hq // hkv
    return ("attention_gqa_rows_kernel", T, bool(causal), 4 if per_kv % 4 == 0 else 2 if per_kv % 2 == 0 else 1)


def all_instantiations() -> set:
    """The 40 instantiations encoder_ops.hip dispatches to."""
    inst = {("attention_short_kernel", T, None, None) for T in (1, 2, 3, 4)} | {("attention_rows_kernel", T, None, None) for T in (5, 6, 7, 8)}
    inst |= {("attention_gqa_kernel", T, c, None) for T in (1, 2, 3, 4) for c in (False, True)}
    inst |= {("attention_gqa_rows_kernel", T, c, R) for T in (5, 6, 7, 8) for c in (False, True) for R in (1, 2, 4)}
    assert len(inst) == 40
    return inst


def reached_instantiations(lengths=LENGTHS) -> set:
    got = {kernel_of("short", S) for S in lengths}
    return got | {kernel_of("gqa", S, hq, hkv, c) for S in lengths for hq, hkv in GQA_HEADS for c in (False, True)}


# ---- small pieces --------------------------------------------------------------------------------------------------------------------
def scale_log2e(hd: int) -> float:
    """The kernels' fp32 constant: float(1 / sqrt(hd)) * float(log2 e), the product rounded to fp32."""
    return float(torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def allowed(mask, B: int, S: int, causal: bool, device=None, strict: bool = False) -> torch.Tensor:
    """[B][S][S] bool: query i may read key k (the key mask, and k <= i under causal; `strict`: k < i, the causal_lt mistake)."""
    allow = torch.ones((B, S, S), dtype=torch.bool, device=device)
    if causal:
        allow = allow & torch.ones((S, S), dtype=torch.bool, device=device).tril_(-1 if strict else 0)[None]
    if mask is not None:
        allow = allow & (mask.to(allow.device)[:, None, :] != 0)
    return allow


def fill_big(t: torch.Tensor, where: torch.Tensor) -> None:
    """Set the bf16 rows of `t` [B][S][...] that `where` [B][S] selects to 0x7F7F, in place."""
    t.view(torch.int16)[where.to(t.device)] = BIG_BITS


def key_codes(hd: int) -> torch.Tensor:
    """[128][hd] fp32: row k is the +-8 code of k's 7 bits, each repeated hd // 7 times, the remaining columns zero."""
    reps = hd // CODE_BITS
    bit = (torch.arange(128)[:, None] >> torch.arange(CODE_BITS)[None, :]) & 1
    code = torch.zeros((128, hd))
    code[:, :CODE_BITS * reps] = (bit.float() * 2.0 - 1.0).repeat_interleave(reps, dim=1) * CODE_VALUE
    return code


def selector_scores(hd: int) -> tuple:
    """(peak, gap) of the construction: a key's score against its own code, and the best wrong key's score minus that (< 0)."""
    code = key_codes(hd)
    s = code.double() @ code.double().T
    peak = s.diagonal()
    assert bool((peak == peak[0]).all())
    off = s - torch.diag(torch.full((128,), float("inf"), dtype=torch.float64))
    return float(peak[0]), float((off - peak[:, None]).max())


def zero_gap(hd: int) -> int:
    """The smallest integer score distance d at which exp2f(-d scale log2e) is exactly 0: the argument is <= -150."""
    return math.ceil(150.0 / scale_log2e(hd))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_inputs(B: int, S: int, hq: int, hkv: int, hd: int):
    """qkv bf16 [B][S][(hq + 2 hkv) hd] ~ N(0, SIGMA[hd]^2) and one mask of each kind of ec.attention_masks, seeded by the shape: the
    GPU file and the CPU file see the same ones."""
    g = ec._gen(7, B, S, hq, hkv, hd)
    qkv = (torch.randn((B, S, (hq + 2 * hkv) * hd), generator=g) * SIGMA[hd]).to(torch.bfloat16)
    return qkv, ec.attention_masks(B, S, g)


def ones_inputs(B: int, S: int, hq: int, hkv: int, hd: int):
    """random_inputs with V = 1 everywhere: every output is the sum of the row's P."""
    qkv, masks = random_inputs(B, S, hq, hkv, hd)
    qkv.view(B, S, hq + 2 * hkv, hd)[:, :, hq + hkv:] = 1.0
    return qkv, masks


def selector_inputs(B: int, S: int, hq: int, hkv: int, hd: int, mask, causal: bool, pick: str, g: torch.Generator):
    """(qkv bf16 [B][S][(hq + 2 hkv) hd], pi int64 [B][S], has_key bool [B][S]) on the CPU: the module docstring's construction.
    pick = "first" / "last" / "random" allowed key of each query row (under causal the last one is the diagonal or the last
    unmasked key before it); rows without an allowed key get key 0's code as their query.  V ~ N(0, 1) from `g`, a different
    row for every (batch, key, key / value head); the K and V rows of the keys the mask excludes hold 0x7F7F."""
    assert pick in PICKS and S <= 128 and hq % hkv == 0
    allow = allowed(mask, B, S, causal)
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
        fill_big(k, mask == 0)
        fill_big(v, mask == 0)
    qkv = torch.cat((q, k, v), dim=2).reshape(B, S, (hq + 2 * hkv) * hd).contiguous()
    return qkv, pi, has_key


def selector_want(qkv: torch.Tensor, pi: torch.Tensor, has_key: torch.Tensor, hq: int, hkv: int, hd: int) -> torch.Tensor:
    """bf16 [B][S][hq hd]: row (b, i) of query head h is V[b, pi(i), h // (hq / hkv)]; rows without an allowed key are zeros."""
    B, S, _ = qkv.shape
    pi, has_key = pi.to(qkv.device), has_key.to(qkv.device)
    v = qkv.view(B, S, hq + 2 * hkv, hd)[:, :, hq + hkv:]
    rows = v[torch.arange(B, device=qkv.device)[:, None], pi]                      # [B][S][hkv][hd]
    rows = rows.repeat_interleave(hq // hkv, dim=2)
    return torch.where(has_key[:, :, None, None], rows, torch.zeros_like(rows)).reshape(B, S, hq * hd)


def pad_right(qkv: torch.Tensor, S: int):
    """The batch re-laid at length S: the extra tokens hold 0x7F7F and the returned mask [B][S] takes them out."""
    B, S0, w = qkv.shape
    out = torch.empty((B, S, w), dtype=qkv.dtype, device=qkv.device)
    out.view(torch.int16)[:] = BIG_BITS
    out[:, :S0] = qkv
    mask = (torch.arange(S, device=qkv.device)[None, :] < S0).to(torch.int64).expand(B, S).contiguous()
    return out, mask


def alone(qkv: torch.Tensor, b: int, hq: int, hkv: int, hd: int, kvh: int) -> torch.Tensor:
    """Sequence b's key / value group kvh as a call of its own: [1][S][(hq / hkv + 2) hd], its query heads, its key, its value head."""
    B, S, _ = qkv.shape
    per_kv = hq // hkv
    x = qkv.view(B, S, hq + 2 * hkv, hd)[b:b + 1]
    return torch.cat((x[:, :, kvh * per_kv:(kvh + 1) * per_kv], x[:, :, hq + kvh:hq + kvh + 1], x[:, :, hq + hkv + kvh:hq + hkv + kvh + 1]),
                     dim=2).reshape(1, S, (per_kv + 2) * hd).contiguous()


# ---- the kernels' arithmetic ---------------------------------------------------------------------------------------------------------------
def emulate(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, *, mutate=None) -> torch.Tensor:
    """bf16 [B][S][hq hd]: the module docstring's model, with the mistake `mutate` names (None: none):
    causal_lt: key < query for key <= query;  drop_last_key: the last allowed key of each row is left out;  drop_tile_edge_key:
    key 16 t of the last tile t is left out;  other_scale: 1 / sqrt(64) and 1 / sqrt(128) swapped;  truncate_p: P cut to bf16, not
    rounded;  kv_head_mod: query head h reads key / value head h % hkv;  swap_key_pair: keys 2 j and 2 j + 1 of V swapped;
    stale_pad: the P columns past S of the last 32-key step hold 1.0 against V[S - 1];  no_max: no max subtraction."""
    assert mutate is None or mutate in MUTANTS, mutate
    B, S, _ = qkv.shape
    dev = qkv.device
    f32 = torch.float32
    heads = torch.arange(hq, device=dev)
    kvh = heads % hkv if mutate == "kv_head_mod" else heads // (hq // hkv)
    x = qkv.view(B, S, hq + 2 * hkv, hd).float()
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv][:, :, kvh], x[:, :, hq + hkv:][:, :, kvh]
    if mutate == "swap_key_pair":
        v = v[:, (torch.arange(S, device=dev) ^ 1).clamp(max=S - 1)]
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k)
    allow = allowed(mask, B, S, causal, dev, strict=mutate == "causal_lt")
    ar = torch.arange(S, device=dev)[None, None, :]
    if mutate == "drop_last_key":
        allow = allow & (ar != torch.where(allow, ar, -1).amax(-1, keepdim=True))
    if mutate == "drop_tile_edge_key":
        allow = allow & (ar != 16 * ((S - 1) // 16))
    allow = allow[:, None]
    sl = scale_log2e(192 - hd if mutate == "other_scale" else hd)
    ninf, zero = torch.tensor(float("-inf"), dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev)
    m = zero if mutate == "no_max" else torch.where(allow, sc, ninf).amax(-1, keepdim=True)
    e = torch.where(allow, torch.exp2((sc - m) * sl), zero)
    tot = e.sum(-1, keepdim=True)
    p = e * torch.where(tot > 0, 1.0 / tot, zero)
    p = (p.view(torch.int32) & -65536).view(f32) if mutate == "truncate_p" else p.to(torch.bfloat16).float()
    acc = torch.einsum("bhqk,bkhd->bqhd", p, v)
    if mutate == "stale_pad":
        acc = acc + float(32 * (-(-S // 32)) - S) * v[:, S - 1][:, None]
    return acc.to(torch.bfloat16).reshape(B, S, hq * hd)


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
    return want, has_key, u * (A + want.abs()) + u * u * A


def bound_ratio(got: torch.Tensor, want: torch.Tensor, has_key: torch.Tensor, bnd: torch.Tensor) -> float:
    """Worst |got - want| / bound over the rows with a key; 1e30 where the error is not finite or a zero bound is missed."""
    if not bool(has_key.any()):
        return 0.0
    err = (got.double() - want).abs()[has_key]
    b = bnd[has_key]
    ratio = torch.where((b == 0) & (err == 0), torch.zeros_like(err), err / b)
    return float(ratio.nan_to_num(nan=1e30, posinf=1e30).max())


def ones_share(got: torch.Tensor, has_key: torch.Tensor) -> float:
    """The share of the elements of the rows with a key that are exactly 1.0 (1.0 for no such row)."""
    rows = got[has_key]
    return float((rows == 1.0).double().mean()) if rows.numel() else 1.0
