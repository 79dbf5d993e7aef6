"""References, bounds, inputs and guarded buffers for the direct tests of the encoder's fp32-path kernels
(tests/test_encoder_ref_cpu.py, test_encoder_pieces_gpu.py, test_encoder_edges_gpu.py, test_encoder_rope_act_gpu.py).  Plain
torch, no library: everything here runs without a GPU, and test_encoder_ref_cpu.py shows that a correct fp32 implementation
passes each bound with room and that each checker rejects the corruptions a wrong kernel would produce.

Bounds (none of them comes from what the kernels return):
* pieces of an activation: |hi + lo - y64| <= 2^-16 |y64| + 2^-20 max(1, |g|) max(1, |u|).  The first term is what two
  bf16 pieces hold (lo rounds a remainder of at most 2^-8 |y| to 2^-8 of itself; tests/test_mirrors_gpu.py uses the same
  2^-16 for ts_split_pieces), the second is 8 fp32 ulps (8 * 2^-23) of the activation's scale: erff / expf / tanhf are good
  to a few ulps and `1 + erf` cancels for negative arguments, where the error stays an ulp of 1 times |g| / 2.
* hi alone: |hi - y64| <= 2^-8 |y64| + the same floor (half a bf16 ulp is at most 2^-8 of the value: hi must be the rounded
  value itself, not a truncated or a neighbouring one).  Exact rounding reaches this bound by itself just above a power of
  two, so it has no factor to spare: only the floor separates it from a correct kernel.
* norms: atol = rtol = 2e-5 (fp32) / 2e-2 (bf16) against fp64, the project's tolerances for these kernels.
* per-head norm + rotary (ts_qk_norm_rope, ts_gemma_qk_norm_rope): per element, against A + B = y cos + rot sin in fp64,
  |got - (A + B)| <= (K u (1 + 2^-6) [+ 2^-20]) (|A| + |B|): K roundings of u each (ROPE_K), second-order terms in the 2^-6,
  and for bf16 2^-20 for the fp32 arithmetic in between (rsqrtf, the 128 / 256-term sum).  An all-zero head has bound 0.
* gated activations (ts_swiglu, ts_geglu): K u |y| [(1 + 2^-6) for bf16] + pieces_floor(g, u), K = 2 roundings in bf16 (the
  activation, the product), GATED_K_F32 in fp32; the floor is the activation's own fp32 error, as for the pieces.
"""
import math

import torch

TS_ERR_INVALID, TS_ERR_NODEVICE, TS_ERR_UNSUPPORTED = -1, -4, -5

# ---- shapes every file uses ---------------------------------------------------------------------------------------------
# one wave per row, 16-byte accesses (4 fp32 / 8 bf16 elements), 1, 2 or 4 of them per lane: 64, 128, 256 accesses per row.
# Each class at its lower edge (one lane holds the last access alone: 65 -> d = 260 / 520, 129 -> 516 / 1032), its full width
# and the width one access short of it; d = 4 / 8 is a single lane.
NORM_WIDTHS_F32 = (4, 252, 256, 260, 512, 516, 768, 1020, 1024)
NORM_WIDTHS_BF16 = (8, 504, 512, 520, 1024, 1032, 2040, 2048)
NORM_ROWS = (1, 5, 259)                      # four rows per workgroup: the last one holds 1, 1 and 3 waves
NORM_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}
LN_EPS, RMS_EPS = 1e-12, 1e-6

ACT_KINDS = (0, 1, 2)
ACT_WIDTHS = (4, 252, 1024, 3072)
ACT_ROWS = (1, 5, 259)
ACT_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 5.5, -5.5, 8.0, -8.0, 30.0, -30.0, 100.0, -100.0)

# the elementwise kernels launch min(ceil(items / 256), 16384) workgroups of 256 threads (encoder_ops.hip) and stride over the
# rest: 16384 * 256 threads.  The smallest item count at which EVERY thread takes a second item is twice that.
GRID_CAP_THREADS = 16384 * 256
GRID_STRIDE_ROWS, GRID_STRIDE_N = 8192, 4096                 # rows * n / 4 = 8,388,608 = 2 * GRID_CAP_THREADS
assert GRID_STRIDE_ROWS * (GRID_STRIDE_N // 4) == 2 * GRID_CAP_THREADS

# per-head norm + rotary: a head is hd / VEC lanes of a wave (16 or 32 in bf16, 32 or 64 in fp32), so a wave holds 4, 2 or 1
# (token, head) items and a workgroup of four waves 16, 8 or 4.  (tokens, seq, q heads, kv heads):
ROPE_SHAPES = ((1, 1, 1, 1),        # 2 items: idle groups or idle waves in the only workgroup
               (3, 3, 2, 1),        # 9 items: one live group in the last wave
               (7, 7, 2, 1),        # 21 items: a second, partial workgroup that ends in idle groups
               (5, 8, 3, 1),        # seq > tokens
               (10, 4, 2, 2),       # tokens not a multiple of seq, hq == hkv
               (6, 1, 4, 4),        # seq == 1
               (259, 7, 3, 1),      # Gemma3's own head counts
               (185, 37, 16, 8))    # Qwen3's own head counts
ROPE_HEAD = {False: 128, True: 256}                          # by `gemma`: ts_qk_norm_rope serves 128, ts_gemma_qk_norm_rope 256
ROPE_EPS = 1e-6
ROPE_HEAD_SCALES = {"zero": 0.0, "small": 1e-4, "big": 300.0}
ROPE_PREFIX_SHAPE, ROPE_PREFIXES = (23, 7, 2, 1), (1, 2, 3, 5, 6, 7, 22)      # 3 heads a token: 3, 6, 9, 15, ... items
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}
# roundings of u each between the stored operands and the stored answer, by (gemma, storage type).
# bf16: Qwen3 x r | w . | the product with cos / sin | the sum;  Gemma3 the norm (rounded once) | the product | the sum.
# fp32: twice what torch's fp32 evaluation of the kernel's sequence (rope_emulate) reaches against rope_ref over ROPE_SHAPES'
# inputs, rounded up: measured 4.83 u (Qwen3) and 5.48 u (Gemma3) of |A| + |B| (tests/test_encoder_ref_cpu.py prints them)
ROPE_K = {(False, torch.bfloat16): 4, (True, torch.bfloat16): 3, (False, torch.float32): 10, (True, torch.float32): 11}

# gated activations: inter of one access (VEC), one access short of a wave's (fp32) / half a wave's (bf16), two ordinary ones
GATED_WIDTHS = {torch.float32: (4, 252, 1024, 3072), torch.bfloat16: (8, 248, 1024, 3072)}
GATED_ROWS = (1, 5, 259)
GATED_STRIDE = {torch.float32: (8192, 4096), torch.bfloat16: (8192, 8192)}   # rows, inter: rows * inter / VEC = 2 * GRID_CAP_THREADS
assert all(r * (n // (16 // torch.empty((), dtype=t).element_size())) == 2 * GRID_CAP_THREADS for t, (r, n) in GATED_STRIDE.items())
# fp32: K u |y| + pieces_floor.  On gated_inputs act_fp32 never leaves the floor (measured: 0 u beyond it, 0.147 (SwiGLU) and
# 0.144 (GeGLU) of the bound below; tests/test_encoder_ref_cpu.py prints them), so twice the measurement would be K = 0.  K is
# the two fp32 roundings the kernel adds to the activation's own error instead: the activation's result and the product.
GATED_K_F32 = {1: 2, 2: 2}


# ---- bf16 pieces ----------------------------------------------------------------------------------------------------------
def split_ref(y: torch.Tensor) -> torch.Tensor:
    """fp32 [rows x k] -> bf16 [rows x 3k] = [hi | lo | hi], hi = bf16(y), lo = bf16(y - hi), torch's CPU rounding."""
    y = y.detach().cpu().float()
    hi = y.bfloat16()
    lo = (y - hi.float()).bfloat16()
    return torch.cat((hi, lo, hi), dim=-1)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of a tensor, for bit-for-bit comparisons (NaN payloads and signed zeros included)."""
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def act_operands(x: torch.Tensor, bias, kind: int):
    """The activation's operands as the kernel forms them: x + bias in fp32; (g, None) for kind 0, (gate, up) otherwise."""
    xb = x.float() if bias is None else x.float() + bias.float()
    if kind == 0:
        return xb, None
    n = xb.shape[-1] // 2
    return xb[..., :n], xb[..., n:]


def act_ref(x: torch.Tensor, bias, kind: int) -> torch.Tensor:
    """fp64 activation of the fp32 operands: kind 0 gelu (erf), 1 silu(gate) * up, 2 gelu_tanh(gate) * up (gate columns first)."""
    g, u = act_operands(x, bias, kind)
    g = g.double()
    if kind == 0:
        return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    if kind == 1:
        return g * torch.sigmoid(g) * u.double()
    if kind == 2:
        return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g * g * g))) * u.double()
    raise ValueError(kind)


def act_fp32(x: torch.Tensor, bias, kind: int) -> torch.Tensor:
    """The same in torch's own fp32: what a correct fp32 implementation returns (the CPU test measures it against the bound)."""
    g, u = act_operands(x, bias, kind)
    F = torch.nn.functional
    return F.gelu(g) if kind == 0 else F.silu(g) * u if kind == 1 else F.gelu(g, approximate="tanh") * u


def pieces_floor(g: torch.Tensor, u) -> torch.Tensor:
    s = g.double().abs().clamp(min=1.0)
    if u is not None:
        s = s * u.double().abs().clamp(min=1.0)
    return 2.0 ** -20 * s


def pieces_bound(y64: torch.Tensor, g: torch.Tensor, u) -> torch.Tensor:
    return 2.0 ** -16 * y64.abs() + pieces_floor(g, u)


def check_act_pieces(pieces: torch.Tensor, x: torch.Tensor, bias, kind: int, bound_scale: float = 1.0) -> dict:
    """Assert that `pieces` bf16 [rows x 3n] are the pieces of act(x + bias): third block == first bit for bit, hi + lo within
    pieces_bound of fp64 on EVERY element, hi alone within one bf16 rounding.  Returns the worst error / bound ratios."""
    pieces, x = pieces.detach().cpu(), x.detach().cpu()
    bias = None if bias is None else bias.detach().cpu()
    y64 = act_ref(x, bias, kind)
    n = y64.shape[-1]
    assert pieces.dtype == torch.bfloat16 and tuple(pieces.shape) == (y64.shape[0], 3 * n), (pieces.dtype, pieces.shape)
    hi, lo, hi2 = pieces[:, :n], pieces[:, n:2 * n], pieces[:, 2 * n:]
    assert same_bits(hi, hi2), "the third block is not the first (layout is [hi | lo | hi])"
    g, u = act_operands(x, bias, kind)
    bound = pieces_bound(y64, g, u) * bound_scale
    err = (hi.double() + lo.double() - y64).abs()
    bad = err > bound                                        # NaN compares false here ...
    assert torch.isfinite(err).all() and not bad.any(), \
        f"hi + lo off: {int(bad.sum()) + int((~torch.isfinite(err)).sum())} of {err.numel()} elements, worst ratio {float((err / bound).nan_to_num(posinf=1e30, nan=1e30).max()):.3g}"
    hbound = 2.0 ** -8 * y64.abs() + pieces_floor(g, u)
    herr = (hi.double() - y64).abs()
    assert not (herr > hbound).any(), f"hi is not the rounded value: worst ratio {float((herr / hbound).max()):.3g}"
    return {"pieces": float((err / bound).max()), "hi": float((herr / hbound).max())}


def check_norm_pieces(out: torch.Tensor, pieces: torch.Tensor, want64: torch.Tensor, tol: float = 2e-5) -> float:
    """Assert that fp32 `out` is within atol = rtol = tol of fp64 `want64` and that `pieces` are split_ref(out) bit for bit.
    Returns the worst error / (tol + tol |want|)."""
    out, pieces, want64 = out.detach().cpu(), pieces.detach().cpu(), want64.detach().cpu()
    assert out.dtype == torch.float32 and out.shape == want64.shape
    ratio = (out.double() - want64).abs() / (tol + tol * want64.abs())
    assert torch.isfinite(ratio).all() and float(ratio.max()) <= 1.0, f"out off: worst error / tolerance {float(ratio.nan_to_num(nan=1e30).max()):.3g}"
    assert same_bits(pieces, split_ref(out)), "pieces are not [hi | lo | hi] of out"
    return float(ratio.max())


def norm_ratio(out: torch.Tensor, want64: torch.Tensor, tol: float) -> float:
    """Worst |out - want| / (tol + tol |want|): <= 1 is torch.allclose(out, want, atol=tol, rtol=tol).  NaN counts as failing."""
    r = (out.detach().double() - want64.to(out.device)).abs() / (tol + tol * want64.to(out.device).abs())
    return float(r.nan_to_num(nan=1e30, posinf=1e30).max())


# ---- seeded inputs (the GPU tests and the CPU reference test use the same ones) ----------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % 2147483647
    return torch.Generator(device="cpu").manual_seed(seed)


def layernorm_inputs(d: int, rows: int, dtype=torch.float32):
    """a, a_bias, b, gamma, beta at the scales of test_add_layernorm_kernel_matches_torch_in_fp64; row 0 of a and b all zeros."""
    g = _gen(1, d, rows)
    a = (torch.randn((rows, d), generator=g) * 2.0 + 0.3).to(dtype)
    b = torch.randn((rows, d), generator=g).to(dtype)
    a[0], b[0] = 0.0, 0.0
    a_bias = (0.5 * torch.randn(d, generator=g)).to(dtype)
    gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).to(dtype)
    beta = (0.1 * torch.randn(d, generator=g)).to(dtype)
    return a, a_bias, b, gamma, beta


def rmsnorm_inputs(d: int, rows: int, dtype=torch.float32):
    """a, b, gamma at the scales of test_add_rmsnorm_kernel_matches_the_module_chain; row 0 of a and b all zeros."""
    g = _gen(2, d, rows)
    a = (torch.randn((rows, d), generator=g) * 1.7).to(dtype)
    b = torch.randn((rows, d), generator=g).to(dtype)
    a[0], b[0] = 0.0, 0.0
    gamma = (1.0 + 0.2 * torch.randn(d, generator=g)).to(dtype)
    return a, b, gamma


def gemma_inputs(d: int, rows: int, dtype=torch.float32):
    """y, x, w_post, w_next at the scales of test_gemma3_kernels_match_the_modules; row 0 of x and y all zeros."""
    g = _gen(3, d, rows)
    x = (torch.randn((rows, d), generator=g) * 3.0).to(dtype)
    y = (torch.randn((rows, d), generator=g) * 0.7).to(dtype)
    x[0], y[0] = 0.0, 0.0
    w_post = (0.3 * torch.randn(d, generator=g)).to(dtype)
    w_next = (0.3 * torch.randn(d, generator=g)).to(dtype)
    return y, x, w_post, w_next


def act_inputs(kind: int, n: int, rows: int):
    """x [rows x n] (kind 0) or [rows x 2n] ~ N(0, 2^2) with the values of ACT_SPECIALS set into every `step`-th column (a
    different one per row and column, gate and up halves alike), and a bias over the input's width."""
    g = _gen(4, kind, n, rows)
    width = n if kind == 0 else 2 * n
    x = torch.randn((rows, width), generator=g) * 2.0
    step = max(2, width // 24)
    cols = torch.arange(0, width, step)
    pick = (torch.arange(rows)[:, None] + torch.arange(len(cols))[None, :]) % len(ACT_SPECIALS)
    x[:, cols] = torch.tensor(ACT_SPECIALS, dtype=torch.float32)[pick]
    bias = torch.randn(width, generator=g)
    return x, bias


def gated_inputs(kind: int, inter: int, rows: int, dtype) -> torch.Tensor:
    """gate_up [rows x 2 inter] of the storage type: act_inputs' values (the specials in gate and up columns alike), no bias."""
    return act_inputs(kind, inter, rows)[0].to(dtype)


def rope_special_heads(tokens: int, hq: int, hkv: int) -> dict:
    """Where rope_inputs puts its special heads: name -> (token, head), head counted over queries then keys.  The all-zero
    head is the last item (the one live group of a last wave), and item 0 stays ordinary; two items hold two specials."""
    heads = hq + hkv
    items = tokens * heads
    at = {"zero": items - 1, "small": items // 2, "big": 1} if items >= 4 else {"zero": 1, "small": 0}
    return {name: divmod(i, heads) for name, i in at.items()}


def rope_inputs(tokens: int, seq: int, hq: int, hkv: int, gemma: bool, dtype):
    """qkv [tokens x (hq + 2 hkv) hd] ~ N(0, 1.3^2) with the heads of rope_special_heads scaled by ROPE_HEAD_SCALES (at 1e-4
    eps = 1e-6 dominates the mean square), wq, wk [hd] = 1 + 0.3 N (Qwen3) / 0.3 N (Gemma3: the kernel adds the 1), cos, sin
    [seq x hd] of an independent uniform angle per (position, element): the two halves of a row differ and no sin is
    systematically small.  All of the storage type."""
    hd = ROPE_HEAD[gemma]
    g = _gen(6, tokens, seq, hq, hkv, int(gemma))
    qkv = torch.randn((tokens, hq + 2 * hkv, hd), generator=g) * 1.3
    for name, (tok, h) in rope_special_heads(tokens, hq, hkv).items():
        qkv[tok, h] = qkv[tok, h] * ROPE_HEAD_SCALES[name] if ROPE_HEAD_SCALES[name] else 0.0      # (+0, not randn's signs)
    wq, wk = ((0.0 if gemma else 1.0) + 0.3 * torch.randn(hd, generator=g) for _ in range(2))
    ang = torch.rand((seq, hd), generator=g) * (2.0 * math.pi)
    return tuple(t.to(dtype).contiguous() for t in (qkv.view(tokens, -1), wq, wk, torch.cos(ang), torch.sin(ang)))


def rope_operands(qkv, wq, wk, cos, sin, seq, hq, hkv, hd, to):
    """x [tokens x heads x hd] (queries, then keys), w [heads x hd], cos / sin [tokens x 1 x hd] at pos = tok % seq, in `to`."""
    tokens = qkv.shape[0]
    x = qkv.view(tokens, hq + 2 * hkv, hd)[:, :hq + hkv].to(to)
    w = torch.cat((wq.to(to).expand(hq, hd), wk.to(to).expand(hkv, hd)))
    pos = torch.arange(tokens, device=qkv.device) % seq
    return x, w, cos.to(to)[pos][:, None, :], sin.to(to)[pos][:, None, :]


def rope_ref(qkv, wq, wk, cos, sin, seq: int, hq: int, hkv: int, hd: int, eps: float, gemma: bool):
    """fp64 on the stored operands, no intermediate rounding: r = rsqrt(mean_hd(x^2) + eps), y = x r w (Qwen3) / x r (1 + w)
    (Gemma3), rot = (-y[hd/2:], y[:hd/2]), A = y cos[pos], B = rot sin[pos], pos = tok % seq.  eps as the fp32 the entry takes.
    Returns (A + B, |A| + |B|) [tokens x (hq + hkv) x hd] fp64 and the value heads [tokens x hkv hd] as stored."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    x, w, c, s = rope_operands(qkv, wq, wk, cos, sin, seq, hq, hkv, hd, torch.float64)
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (1.0 + w if gemma else w)
    rot = torch.cat((-y[..., hd // 2:], y[..., :hd // 2]), dim=-1)
    A, B = y * c, rot * s
    return A + B, A.abs() + B.abs(), qkv[:, (hq + hkv) * hd:]


def rope_emulate(qkv, wq, wk, cos, sin, seq: int, hq: int, hkv: int, hd: int, eps: float, gemma: bool) -> torch.Tensor:
    """The kernel's own sequence in torch (kernels_encoder.h, qk_norm_rope_kernel): fp32 arithmetic, rounded to the storage type
    where the kernel rounds - y = round(w round(x r)) (Qwen3) / round((x r)(1 + w)) (Gemma3), out = round(round(y cos) +
    round(rot sin)).  Returns the whole qkv in the storage type, value heads copied."""
    def rd(t):
        return t.to(qkv.dtype).float()
    x, w, c, s = rope_operands(qkv, wq, wk, cos, sin, seq, hq, hkv, hd, torch.float32)
    r = torch.rsqrt((x * x).sum(-1, keepdim=True) / float(hd) + torch.tensor(eps, dtype=torch.float32))
    y = rd((x * r) * (1.0 + w)) if gemma else rd(w * rd(x * r))
    rot = torch.cat((-y[..., hd // 2:], y[..., :hd // 2]), dim=-1)
    out = qkv.clone()
    out.view(qkv.shape[0], hq + 2 * hkv, hd)[:, :hq + hkv] = (rd(y * c) + rd(rot * s)).to(qkv.dtype)
    return out


def rope_bound(mag: torch.Tensor, dtype, gemma: bool) -> torch.Tensor:
    rel = ROPE_K[(bool(gemma), dtype)] * UNIT[dtype] * (1.0 + 2.0 ** -6)
    return (rel + (2.0 ** -20 if dtype == torch.bfloat16 else 0.0)) * mag     # fp32: ROPE_K is measured with the fp32 parts in it


def rope_ratio(got, qkv, wq, wk, cos, sin, seq: int, hq: int, hkv: int, hd: int, eps: float, gemma: bool) -> torch.Tensor:
    """error / bound per query / key element [tokens x (hq + hkv) x hd]; 0 where a zero bound is met exactly, 1e30 where the
    error is not finite or a zero bound is missed."""
    got, qkv, wq, wk, cos, sin = (t.detach().cpu() for t in (got, qkv, wq, wk, cos, sin))
    want, mag, _ = rope_ref(qkv, wq, wk, cos, sin, seq, hq, hkv, hd, eps, gemma)
    err = (got.view(got.shape[0], hq + 2 * hkv, hd)[:, :hq + hkv].double() - want).abs()
    ratio = (err / rope_bound(mag, qkv.dtype, gemma)).nan_to_num(nan=1e30, posinf=1e30)
    return torch.where((mag == 0) & (err == 0), torch.zeros_like(ratio), ratio)


def check_rope(got, qkv, wq, wk, cos, sin, seq: int, hq: int, hkv: int, hd: int, eps: float, gemma: bool, bound_scale: float = 1.0) -> float:
    """Assert that `got` is the in-place answer for `qkv`: every query / key element within rope_bound, the value heads bit for
    bit the input's, no NaN, the all-zero head zeros.  Returns the worst error / bound."""
    assert got.shape == qkv.shape and got.dtype == qkv.dtype, (got.shape, got.dtype)
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} NaN"
    assert same_bits(got[:, (hq + hkv) * hd:], qkv[:, (hq + hkv) * hd:]), "the value heads changed"
    ratio = rope_ratio(got, qkv, wq, wk, cos, sin, seq, hq, hkv, hd, eps, gemma) / bound_scale
    worst = float(ratio.max())
    assert worst <= 1.0, f"{int((ratio > 1).sum())} of {ratio.numel()} elements off, worst error / bound {worst:.3g}, first at (token, head, element) {tuple(int(i) for i in (ratio > 1).nonzero()[0])}"
    tok, h = rope_special_heads(qkv.shape[0], hq, hkv)["zero"]
    assert not got.view(got.shape[0], hq + 2 * hkv, hd)[tok, h].any(), "the all-zero head is not zeros"
    return worst


def gated_bound(y64: torch.Tensor, g: torch.Tensor, u: torch.Tensor, kind: int, dtype) -> torch.Tensor:
    rel = 2.0 * UNIT[dtype] * (1.0 + 2.0 ** -6) if dtype == torch.bfloat16 else GATED_K_F32[kind] * UNIT[dtype]
    return rel * y64.abs() + pieces_floor(g, u)


def gated_ratio(out: torch.Tensor, gate_up: torch.Tensor, kind: int) -> torch.Tensor:
    """error / bound per element of `out` [rows x inter] for gate_up [rows x 2 inter] (both of the storage type), kind 1 SwiGLU /
    2 GeGLU; 1e30 where the error is not finite."""
    out, gate_up = out.detach().cpu(), gate_up.detach().cpu()
    assert out.dtype == gate_up.dtype and tuple(out.shape) == (gate_up.shape[0], gate_up.shape[1] // 2), (out.dtype, out.shape)
    y64 = act_ref(gate_up, None, kind)
    g, u = act_operands(gate_up, None, kind)
    return ((out.double() - y64).abs() / gated_bound(y64, g, u, kind, out.dtype)).nan_to_num(nan=1e30, posinf=1e30)


def check_gated(out: torch.Tensor, gate_up: torch.Tensor, kind: int, bound_scale: float = 1.0) -> float:
    """Assert that every element of `out` is within gated_bound of the fp64 activation and none is NaN.  Returns the worst ratio."""
    assert not torch.isnan(out).any(), f"{int(torch.isnan(out).sum())} NaN"
    ratio = gated_ratio(out, gate_up, kind) / bound_scale
    worst = float(ratio.max())
    assert worst <= 1.0, f"{int((ratio > 1).sum())} of {ratio.numel()} elements off, worst error / bound {worst:.3g}"
    return worst


# ---- fp64 references of the norms ------------------------------------------------------------------------------------------------
def layernorm_ref(a, a_bias, b, gamma, beta, eps=LN_EPS):
    x = a.double() + b.double() if a_bias is None else a.double() + a_bias.double() + b.double()
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps)


def rmsnorm_ref(a, b, gamma, eps=RMS_EPS):
    """Qwen3's chain: s = a + b rounded to the storage type (torch's own add), out = s rsqrt(mean(s^2) + eps) gamma in fp64.
    Returns (s in the storage type, out fp64)."""
    s = a if b is None else a + b
    s64 = s.double()
    return s, s64 * torch.rsqrt((s64 * s64).mean(-1, keepdim=True) + eps) * gamma.double()


def gemma_ref(y, x, w_post, w_next, eps=RMS_EPS):
    """Gemma3's sandwich: s = x + norm(y; w_post) (s = x without y), h = norm(s; w_next), norm(v; w) = v rsqrt(mean(v^2) + eps)
    (1 + w), all in fp64.  Returns (s, h)."""
    def norm(v, w):
        return v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps) * (1.0 + w.double())
    s = x.double() if y is None else x.double() + norm(y.double(), w_post)
    return s, norm(s, w_next)


def layernorm_fp32(a, a_bias, b, gamma, beta, eps=LN_EPS):
    x = a + b if a_bias is None else (a + a_bias) + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def rmsnorm_fp32(a, b, gamma, eps=RMS_EPS):
    s = a if b is None else a + b
    return s * torch.rsqrt((s * s).mean(-1, keepdim=True) + eps) * gamma


def gemma_fp32(y, x, w_post, w_next, eps=RMS_EPS):
    def norm(v, w):
        return v * torch.rsqrt((v * v).mean(-1, keepdim=True) + eps) * (1.0 + w)
    s = x if y is None else x + norm(y, w_post)
    return s, norm(s, w_next)


def embed_layernorm_ref(ids, type_ids, word, pos, typ, gamma, beta, seq, eps=LN_EPS):
    """BertEmbeddings in fp64: LayerNorm(word[ids] + type[type_ids or 0] + pos[i % seq]); ids flat [tokens]."""
    p = torch.arange(ids.numel(), device=ids.device) % seq
    x = word.double()[ids] + (typ.double()[type_ids] if type_ids is not None else typ.double()[0]) + pos.double()[p]
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps)


# ---- pooling --------------------------------------------------------------------------------------------------------------------
def pool_ref(hidden, mask, pooling: int, normalize: bool):
    """fp64: pooling 0 = sum of unmasked tokens / max(count, 1e-9) (a row without a token: zeros), 1 = the last unmasked token,
    2 = token 0; then x / max(|x|, 1e-12) when `normalize`."""
    hf, mf = hidden.double(), mask.unsqueeze(-1).double()
    n, S = mask.shape
    if pooling == 0:
        ref = (hf * mf).sum(1) / mf.sum(1).clamp(min=1e-9)
    elif pooling == 1:
        last = (mask != 0).long().mul(torch.arange(S, device=mask.device)[None, :]).amax(1)
        ref = hf[torch.arange(n, device=mask.device), last]
    else:
        ref = hf[:, 0]
    return torch.nn.functional.normalize(ref, p=2, dim=1, eps=1e-12) if normalize else ref


def pool_masks(n: int, S: int, seed: int):
    """Left padding with random lengths >= 1 (one row full), and the same with holes punched into the kept tokens and the tail cut
    at a random kept position (at least one token stays in every row)."""
    g = _gen(5, n, S, seed)
    lens = torch.randint(1, S + 1, (n,), generator=g)
    lens[0] = S
    left = (torch.arange(S)[None, :] >= (S - lens)[:, None]).to(torch.int64)
    holes = left * (torch.rand((n, S), generator=g) < 0.6).to(torch.int64)
    # the last kept token of a holed row is a random position of its kept range, not S - 1: "last unmasked" and "last position"
    # differ (and that token is kept, so no row is empty)
    end = (S - lens) + (torch.rand(n, generator=g) * lens).long().clamp(max=lens - 1)
    holes = holes * (torch.arange(S)[None, :] <= end[:, None]).to(torch.int64)
    holes[torch.arange(n), end] = 1
    return left, holes


# ---- attention -------------------------------------------------------------------------------------------------------------------
ATTN_MASK_KINDS = ("none", "right", "left", "holes", "single", "keyless")


def attention_masks(B: int, S: int, g: torch.Generator) -> dict:
    """One key mask [B x S] int64 of each kind (None for "none"): right / left padding with random lengths >= 1 on every
    sequence, random holes (key 0 kept), one sequence with a single key, one sequence with no key at all."""
    ar = torch.arange(S)[None, :]
    lens = torch.randint(1, S + 1, (B,), generator=g)
    right = (ar < lens[:, None]).to(torch.int64)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    left = (ar >= (S - lens)[:, None]).to(torch.int64)
    holes = (torch.rand((B, S), generator=g) < 0.5).to(torch.int64)
    holes[:, 0] = 1
    single = right.clone()
    single[B // 2] = 0
    single[B // 2, int(torch.randint(0, S, (1,), generator=g))] = 1
    keyless = left.clone()
    keyless[B - 1] = 0
    return {"none": None, "right": right, "left": left, "holes": holes, "single": single, "keyless": keyless}


def attention_ref(qkv, mask, hq: int, hkv: int, hd: int, causal: bool, scale: float, bias=None):
    """softmax(Q K^T scale + key mask [+ causal]) V in fp64 from qkv [B x S x (hq + 2 hkv) hd] (+ bias, added in fp32 as the kernel
    does); query head h reads key / value head h // (hq // hkv).  A query row without an allowed key is zeros.
    Returns (context fp64 [B x S x hq hd], has_key bool [B x S])."""
    if bias is not None:
        qkv = qkv + bias
    B, S, _ = qkv.shape
    dev = qkv.device
    q = qkv[..., :hq * hd].view(B, S, hq, hd).double()
    k = qkv[..., hq * hd:(hq + hkv) * hd].view(B, S, hkv, hd).double().repeat_interleave(hq // hkv, dim=2)
    v = qkv[..., (hq + hkv) * hd:].view(B, S, hkv, hd).double().repeat_interleave(hq // hkv, dim=2)
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    allow = torch.ones((B, 1, S, S), dtype=torch.bool, device=dev)
    if causal:
        allow = allow & torch.ones((S, S), dtype=torch.bool, device=dev).tril_()[None, None]
    if mask is not None:
        allow = allow & (mask.to(dev)[:, None, None, :] != 0)
    has_key = allow.any(dim=-1, keepdim=True)                              # [B][1][S][1]
    sc = sc.masked_fill(~allow, float("-inf"))
    p = torch.softmax(sc.masked_fill(~has_key, 0.0), dim=-1)               # (no NaN rows on the way)
    p = torch.where(has_key & allow, p, torch.zeros_like(p))
    want = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(B, S, hq * hd)
    return want, has_key[:, 0, :, 0]


# ---- guarded output buffers -----------------------------------------------------------------------------------------------------
_SENTINEL = 0xFF                                                            # every element reads as NaN in fp32 and in bf16


def guarded(shape, dtype, device="cuda", align: int = 16) -> torch.Tensor:
    """An output tensor of `shape` cut from a larger buffer filled with 0xFF bytes (NaN in fp32 and bf16, so an element the kernel
    did not write fails every comparison), with one row (the last dimension, rounded up to `align` bytes: 16 keeps the kernels'
    16-byte alignment, 8 gives pieces their weakest allowed one) of margin before and after.  `assert_margins` checks them."""
    item = torch.empty((), dtype=dtype).element_size()
    total = 1
    for s in shape:
        total *= int(s)
    margin = -(-int(shape[-1]) * item // align) * align
    raw = torch.full((margin + total * item + margin,), _SENTINEL, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0
    t = raw[margin:margin + total * item].view(dtype).view(*shape)
    t._guard = (raw, margin, total * item)
    return t


def assert_margins(*tensors) -> None:
    """The bytes in front of and behind each guarded tensor still hold the sentinel: nothing wrote outside it."""
    for t in tensors:
        raw, margin, body = t._guard
        front, back = raw[:margin], raw[margin + body:]
        assert bool((front == _SENTINEL).all()), f"{int((front != _SENTINEL).sum())} bytes written in front of the output"
        assert bool((back == _SENTINEL).all()), f"{int((back != _SENTINEL).sum())} bytes written behind the output"


def untouched(t: torch.Tensor) -> bool:
    """Every byte of `t` (a slice of a guarded tensor, e.g. the columns past d of a padded output) still holds the sentinel."""
    return bool((bits(t.contiguous()).view(torch.uint8) == _SENTINEL).all())
