"""What the GPU tests of the encoder's fp32-path kernels rest on, checked without a GPU (tests/encoder_common.py):
* the references pass their own bounds: on the inputs of tests/test_encoder_pieces_gpu.py torch's own fp32 evaluation of each
  formula, split into pieces by split_ref, passes the bound the GPU test uses - with a factor 2 to spare; so do the gated
  activations cast to the storage type and, in fp32, torch's emulation of the rotary kernel's arithmetic on the inputs of
  tests/test_encoder_rope_act_gpu.py (in bf16 that emulation performs every rounding the bound counts and passes the bound);
* the checks have teeth: each corrupted answer a wrong kernel could give is rejected;
* the argument contract of every encoder entry point: every refusal returns before the device check (the library loads
  without a device; a refusal never dereferences a pointer, so aligned fake ones do).
The measured ratios and the rejected corruptions are printed (also without -s)."""
import ctypes as C

import pytest
import torch

import encoder_common as ec
from conftest import gpu_available
from theoremsearch_amd import _ffi

P = 0x7F0000001000                                            # a 16-byte aligned address no refusal dereferences


def _say(capsys, text):
    with capsys.disabled():
        print("\n" + text, end="")


# ---- the references pass their own bounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ec.ACT_KINDS)
def test_fp32_activation_split_by_the_reference_passes_half_the_pieces_bound(kind, capsys):
    worst = {"pieces": 0.0, "hi": 0.0}
    for n in ec.ACT_WIDTHS:
        for rows in ec.ACT_ROWS:
            x, bias = ec.act_inputs(kind, n, rows)
            for b in (None, bias):
                r = ec.check_act_pieces(ec.split_ref(ec.act_fp32(x, b, kind)), x, b, kind, bound_scale=0.5)
                worst = {k: max(worst[k], r[k]) for k in worst}
    # `pieces` is measured against the halved bound; `hi` against the whole one (half a bf16 ulp reaches 2^-8 of the value by itself)
    _say(capsys, f"act kind {kind}: torch fp32 + split_ref reaches {worst['pieces'] / 2:.3f} of pieces_bound, hi alone {worst['hi']:.3f} of its bound")
    assert worst["pieces"] <= 1.0 and worst["hi"] <= 1.0


def test_hi_alone_fails_the_pieces_bound_by_two_orders(capsys):
    """The bound separates two pieces from one: hi alone is off by up to 2^-8 |y|, 256 times what hi + lo may be."""
    x, bias = ec.act_inputs(1, 1024, 259)
    y64 = ec.act_ref(x, bias, 1)
    g, u = ec.act_operands(x, bias, 1)
    hi = ec.act_fp32(x, bias, 1).bfloat16().double()
    ratio = (hi - y64).abs() / ec.pieces_bound(y64, g, u)
    _say(capsys, f"hi alone: worst {float(ratio.max()):.0f} x pieces_bound, over it on {float((ratio > 1).float().mean()):.1%} of elements")
    assert float(ratio.max()) > 100 and float((ratio > 1).float().mean()) > 0.9


def test_fp32_norms_pass_half_the_tolerance_at_every_width(capsys):
    worst = {"layernorm": 0.0, "layernorm+a_bias": 0.0, "rmsnorm": 0.0, "rmsnorm, no addend": 0.0, "gemma": 0.0, "gemma, no y": 0.0}
    tol = ec.NORM_TOL[torch.float32]
    for d in sorted(set(ec.NORM_WIDTHS_F32) | {8}):
        for rows in ec.NORM_ROWS:
            a, a_bias, b, gamma, beta = ec.layernorm_inputs(d, rows)
            worst["layernorm"] = max(worst["layernorm"], ec.norm_ratio(ec.layernorm_fp32(a, None, b, gamma, beta), ec.layernorm_ref(a, None, b, gamma, beta), tol))
            worst["layernorm+a_bias"] = max(worst["layernorm+a_bias"],
                                            ec.norm_ratio(ec.layernorm_fp32(a, a_bias, b, gamma, beta), ec.layernorm_ref(a, a_bias, b, gamma, beta), tol))
            assert torch.equal(ec.layernorm_ref(a, None, b, gamma, beta)[0], beta.double())          # the all-zero row: exactly beta
            a, b, gamma = ec.rmsnorm_inputs(d, rows)
            worst["rmsnorm"] = max(worst["rmsnorm"], ec.norm_ratio(ec.rmsnorm_fp32(a, b, gamma), ec.rmsnorm_ref(a, b, gamma)[1], tol))
            worst["rmsnorm, no addend"] = max(worst["rmsnorm, no addend"], ec.norm_ratio(ec.rmsnorm_fp32(a, None, gamma), ec.rmsnorm_ref(a, None, gamma)[1], tol))
            assert not ec.rmsnorm_ref(a, b, gamma)[1][0].any()                                      # the all-zero row: zeros
            y, x, wp, wn = ec.gemma_inputs(d, rows)
            for yy, name in ((y, "gemma"), (None, "gemma, no y")):
                s32, h32 = ec.gemma_fp32(yy, x, wp, wn)
                s64, h64 = ec.gemma_ref(yy, x, wp, wn)
                worst[name] = max(worst[name], ec.norm_ratio(s32, s64, tol), ec.norm_ratio(h32, h64, tol))
            assert not ec.gemma_ref(y, x, wp, wn)[1][0].any()
    _say(capsys, "torch fp32 norms against fp64, worst error / (2e-5 + 2e-5 |want|): " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.5


def test_fp32_attention_and_pooling_references_agree_with_torch(capsys):
    """attention_ref against torch's own fp32 attention at half the GPU test's 2e-5, keyless rows exactly zero; pool_ref against
    the fp32 expression at half of 1e-5."""
    g = torch.Generator(device="cpu").manual_seed(5)
    worst = 0.0
    for hq, hkv, hd, S in ((4, 2, 64, 33), (2, 1, 128, 17), (3, 1, 256, 16)):
        qkv = torch.randn(3, S, (hq + 2 * hkv) * hd, generator=g) * 1.5
        for kind, mask in ec.attention_masks(3, S, g).items():
            for causal in (False, True):
                want, has_key = ec.attention_ref(qkv, mask, hq, hkv, hd, causal, hd ** -0.5)
                assert not want[~has_key].any()
                if kind == "keyless":
                    assert not has_key[2].any()
                q = qkv[..., :hq * hd].view(3, S, hq, hd).transpose(1, 2)
                k = qkv[..., hq * hd:(hq + hkv) * hd].view(3, S, hkv, hd).transpose(1, 2).repeat_interleave(hq // hkv, dim=1)
                v = qkv[..., (hq + hkv) * hd:].view(3, S, hkv, hd).transpose(1, 2).repeat_interleave(hq // hkv, dim=1)
                allow = torch.ones(3, 1, S, S, dtype=torch.bool)
                if causal:
                    allow = allow & torch.ones(S, S, dtype=torch.bool).tril_()
                if mask is not None:
                    allow = allow & (mask[:, None, None, :] != 0)
                sc = (q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(~allow, -1e30)
                got = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(3, S, hq * hd)
                worst = max(worst, float((got.double() - want)[has_key].abs().max()) / 2e-5)
    _say(capsys, f"torch fp32 attention against attention_ref: worst error {worst:.3f} of 2e-5")
    assert worst <= 0.5
    hidden = torch.randn(5, 19, 100, generator=g)
    left, holes = ec.pool_masks(5, 19, 0)
    holes[2] = 0                                              # a row without a token: zeros under MEAN
    for mask in (left, holes):
        for pooling in (0, 1, 2):
            for normalize in (False, True):
                want = ec.pool_ref(hidden, mask, pooling, normalize)
                m = mask.unsqueeze(-1).float()
                got = ((hidden * m).sum(1) / m.sum(1).clamp(min=1e-9) if pooling == 0 else
                       hidden[torch.arange(5), (mask * torch.arange(19)[None]).amax(1)] if pooling == 1 else hidden[:, 0])
                got = torch.nn.functional.normalize(got, dim=1) if normalize else got
                assert torch.allclose(got.double(), want, atol=5e-6, rtol=5e-6)
    assert not ec.pool_ref(hidden, holes, 0, True)[2].any() and not ec.pool_ref(hidden, holes, 0, False)[2].any()


F32, BF16 = torch.float32, torch.bfloat16
ROPE_CASES = [(gemma, dtype) for gemma in (False, True) for dtype in (F32, BF16)]
ROPE_IDS = [f"{'gemma3' if gemma else 'qwen3'}-{'fp32' if dtype == F32 else 'bf16'}" for gemma, dtype in ROPE_CASES]


@pytest.mark.parametrize("gemma,dtype", ROPE_CASES, ids=ROPE_IDS)
def test_the_kernels_arithmetic_in_torch_passes_the_rotary_bound(gemma, dtype, capsys):
    """rope_emulate (the kernel's sequence and rounding points, torch's fp32) against rope_ref on every input of the GPU test.
    fp32: half the bound - ROPE_K is twice what this test measures, and the printed figure is that measurement.  bf16: the
    bound itself.  It counts the K roundings of the sequence at their worst case of u each and the emulation performs all K,
    so it comes close (0.79 Qwen3, 0.90 Gemma3) and nothing like a factor 2 is left; the corruptions below miss by far more."""
    hd = ec.ROPE_HEAD[gemma]
    worst, heads = 0.0, {}
    for tokens, seq, hq, hkv in ec.ROPE_SHAPES + (ec.ROPE_PREFIX_SHAPE,):
        ins = ec.rope_inputs(tokens, seq, hq, hkv, gemma, dtype)
        got = ec.rope_emulate(*ins, seq, hq, hkv, hd, ec.ROPE_EPS, gemma)
        worst = max(worst, ec.check_rope(got, *ins, seq, hq, hkv, hd, ec.ROPE_EPS, gemma))
        ratio = ec.rope_ratio(got, *ins, seq, hq, hkv, hd, ec.ROPE_EPS, gemma)
        for name, (tok, h) in ec.rope_special_heads(tokens, hq, hkv).items():
            heads[name] = max(heads.get(name, 0.0), float(ratio[tok, h].max()))
    K = ec.ROPE_K[(gemma, dtype)]
    _say(capsys, f"rotary {ROPE_IDS[ROPE_CASES.index((gemma, dtype))]}: torch's emulation reaches {worst:.3f} of the bound (K = {K}) = "
                 f"{worst * K * (1 + 2.0 ** -6):.2f} u (|A| + |B|); heads scaled by 1e-4 {heads['small']:.3f}, by 300 {heads['big']:.3f}, zero {heads['zero']:.0f}")
    assert set(heads) == {"zero", "small", "big"} and heads["zero"] == 0.0
    assert worst <= (0.5 if dtype == F32 else 1.0)


@pytest.mark.parametrize("kind", (1, 2))
def test_fp32_gated_activation_cast_to_the_storage_type_passes_half_the_bound(kind, capsys):
    worst = {F32: 0.0, BF16: 0.0}
    beyond = 0.0
    for dtype in worst:
        for inter in ec.GATED_WIDTHS[dtype]:
            for rows in ec.GATED_ROWS:
                x = ec.gated_inputs(kind, inter, rows, dtype)
                out = ec.act_fp32(x, None, kind).to(dtype)
                worst[dtype] = max(worst[dtype], ec.check_gated(out, x, kind, bound_scale=0.5) / 2.0)
                if dtype == F32:                              # what GATED_K_F32 would be measured from: the error the floor leaves over
                    y64 = ec.act_ref(x, None, kind)
                    over = ((out.double() - y64).abs() - ec.pieces_floor(*ec.act_operands(x, None, kind))).clamp(min=0.0)
                    beyond = max(beyond, float((over / (ec.UNIT[F32] * y64.abs()).clamp(min=1e-300)).max()))
    _say(capsys, f"{'SwiGLU' if kind == 1 else 'GeGLU'}: torch fp32 cast to the storage type reaches {worst[F32]:.3f} (fp32, K = {ec.GATED_K_F32[kind]}; "
                 f"{beyond:.2f} u |y| beyond the floor) and {worst[BF16]:.3f} (bf16) of the bound")
    assert max(worst.values()) <= 0.5


# ---- the checks have teeth -------------------------------------------------------------------------------------------------------
def _thirds(p):
    n = p.shape[1] // 3
    return p[:, :n], p[:, n:2 * n], p[:, 2 * n:]


def _corrupt_act(name, kind, x, bias):
    """The pieces a kernel with defect `name` would return for act(x + bias); None where the defect does not exist for `kind`."""
    y = ec.act_fp32(x, bias, kind)
    n = y.shape[1]
    hi, lo, _ = _thirds(ec.split_ref(y))
    if name == "[hi | hi | lo] in place of [hi | lo | hi]":
        return torch.cat((hi, hi, lo), dim=1)
    if name == "lo zeroed":
        return torch.cat((hi, torch.zeros_like(lo), hi), dim=1)
    if name == "gate and up halves swapped":
        return None if kind == 0 else ec.split_ref(ec.act_fp32(torch.cat((x[:, n:], x[:, :n]), dim=1), torch.cat((bias[n:], bias[:n])), kind))
    if name == "the up half's bias taken from the gate's columns":
        return None if kind == 0 else ec.split_ref(ec.act_fp32(x, torch.cat((bias[:n], bias[:n])), kind))
    if name == "one 4-element chunk shifted by one chunk":
        y = y.clone()
        y[:, 8:12] = y[:, 4:8].clone()
        return ec.split_ref(y)
    if name == "row r written at row r + 1":
        return ec.split_ref(torch.roll(y, 1, dims=0))
    raise ValueError(name)


CORRUPTIONS = ("[hi | hi | lo] in place of [hi | lo | hi]", "lo zeroed", "gate and up halves swapped",
               "the up half's bias taken from the gate's columns", "one 4-element chunk shifted by one chunk", "row r written at row r + 1")


@pytest.mark.parametrize("name", CORRUPTIONS)
def test_the_checkers_reject_a_corrupted_answer(name, capsys):
    rejected = []
    for kind in ec.ACT_KINDS:
        x, bias = ec.act_inputs(kind, 252, 5)
        ec.check_act_pieces(ec.split_ref(ec.act_fp32(x, bias, kind)), x, bias, kind)               # the right answer passes
        bad = _corrupt_act(name, kind, x, bias)
        if bad is None:
            continue
        with pytest.raises(AssertionError):
            ec.check_act_pieces(bad, x, bias, kind)
        rejected.append(f"act kind {kind}")
    # the norm producers' checker (out against fp64, pieces == split_ref(out)): the defects that exist without a gate / up pair
    a, a_bias, b, gamma, beta = ec.layernorm_inputs(260, 5)
    out, want = ec.layernorm_fp32(a, a_bias, b, gamma, beta), ec.layernorm_ref(a, a_bias, b, gamma, beta)
    ec.check_norm_pieces(out, ec.split_ref(out), want)
    hi, lo, _ = _thirds(ec.split_ref(out))
    shifted = out.clone()
    shifted[:, 8:12] = out[:, 4:8]
    bad = {"[hi | hi | lo] in place of [hi | lo | hi]": [(out, torch.cat((hi, hi, lo), dim=1))],
           "lo zeroed": [(out, torch.cat((hi, torch.zeros_like(lo), hi), dim=1))],
           "one 4-element chunk shifted by one chunk": [(shifted, ec.split_ref(shifted)), (out, ec.split_ref(shifted))],
           "row r written at row r + 1": [(torch.roll(out, 1, dims=0), ec.split_ref(torch.roll(out, 1, dims=0))),
                                          (out, ec.split_ref(torch.roll(out, 1, dims=0)))]}.get(name, [])
    for o, p in bad:
        with pytest.raises(AssertionError):
            ec.check_norm_pieces(o, p, want)
    if bad:
        rejected.append("norm out / pieces")
    _say(capsys, f"rejected: {name} ({', '.join(rejected)})")
    assert rejected


def test_an_unwritten_or_overrun_guarded_buffer_is_noticed():
    t = ec.guarded((5, 12), torch.float32, device="cpu")
    p = ec.guarded((5, 36), torch.bfloat16, device="cpu", align=8)
    assert t.data_ptr() % 16 == 0 and p.data_ptr() % 8 == 0 and torch.isnan(t).all() and torch.isnan(p.float()).all()
    ec.assert_margins(t, p)
    assert ec.untouched(t[:, 8:])
    t.zero_()
    ec.assert_margins(t)
    assert not ec.untouched(t[:, 8:])
    raw, margin, body = t._guard
    raw[margin + body] = 0                                     # one byte past the end
    with pytest.raises(AssertionError):
        ec.assert_margins(t)
    raw, margin, body = p._guard
    raw[margin - 1] = 0                                        # one byte in front
    with pytest.raises(AssertionError):
        ec.assert_margins(p)


ROPE_TEETH_SHAPE = (10, 4, 2, 2)                               # tok // seq differs from tok % seq; all three special heads
ROPE_CORRUPTIONS = ("rotation sign flipped", "cos / sin of the partner element (i +- hd / 2)", "eps dropped", "pos = tok // seq",
                    "the key weight on the query heads", "w and 1 + w exchanged", "one value element changed")


def _corrupt_rope(name, qkv, wq, wk, cos, sin, seq, hq, hkv, hd, gemma):
    """The answer (fp64, rounded once to the storage type) of a kernel with defect `name`; None: of a correct one."""
    tokens, heads = qkv.shape[0], hq + hkv
    x, w, c, s = ec.rope_operands(qkv, wq, wk, cos, sin, seq, hq, hkv, hd, torch.float64)
    eps, sign, one = float(torch.tensor(ec.ROPE_EPS, dtype=F32)), 1.0, 1.0 if gemma else 0.0
    if name == "rotation sign flipped":
        sign = -1.0
    elif name == "cos / sin of the partner element (i +- hd / 2)":
        c, s = c.roll(hd // 2, -1), s.roll(hd // 2, -1)
    elif name == "eps dropped":
        eps = 0.0
    elif name == "pos = tok // seq":
        pos = torch.arange(tokens) // seq
        c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    elif name == "the key weight on the query heads":
        w = wk.double().expand(heads, hd)
    elif name == "w and 1 + w exchanged":
        one = 1.0 - one
    y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (one + w)
    rot = sign * torch.cat((-y[..., hd // 2:], y[..., :hd // 2]), dim=-1)
    out = qkv.clone()
    out.view(tokens, hq + 2 * hkv, hd)[:, :heads] = (y * c + rot * s).to(qkv.dtype)
    if name == "one value element changed":
        ec.bits(out)[tokens // 2, heads * hd + 5] ^= 1         # the last bit of one element of the first value head
    return out


@pytest.mark.parametrize("name", ROPE_CORRUPTIONS)
def test_the_rotary_check_rejects_a_corrupted_answer(name, capsys):
    tokens, seq, hq, hkv = ROPE_TEETH_SHAPE
    scored = []
    for gemma, dtype in ROPE_CASES:
        hd = ec.ROPE_HEAD[gemma]
        ins = ec.rope_inputs(tokens, seq, hq, hkv, gemma, dtype)
        shape = (seq, hq, hkv, hd, ec.ROPE_EPS, gemma)
        ec.check_rope(_corrupt_rope(None, *ins, *shape[:4], gemma), *ins, *shape)                    # the right answer passes
        bad = _corrupt_rope(name, *ins, *shape[:4], gemma)
        with pytest.raises(AssertionError):
            ec.check_rope(bad, *ins, *shape)
        ratio = ec.rope_ratio(bad, *ins, *shape)
        if name == "eps dropped":                             # the head where eps dominates the mean square must show it
            tok, h = ec.rope_special_heads(tokens, hq, hkv)["small"]
            ratio = ratio[tok, h]
        if name == "one value element changed":
            assert float(ratio.max()) <= 1.0                   # (the value heads' own check caught it)
            scored.append("the value heads' comparison")
            continue
        assert float(ratio.max()) > 1.0
        scored.append(f"{float(ratio.max()):.3g} x bound, {float((ratio > 1).float().mean()):.0%} of elements")
    _say(capsys, f"rotary, rejected: {name} (" + "; ".join(f"{i}: {s}" for i, s in zip(ROPE_IDS, scored)) + ")")


GATED_CORRUPTIONS = ("gate and up columns swapped", "erf GELU in place of the tanh form", "SiLU without its g factor")


@pytest.mark.parametrize("name", GATED_CORRUPTIONS)
def test_the_gated_check_rejects_a_corrupted_answer(name, capsys):
    scored = []
    for kind in (1, 2):
        for dtype in (F32, BF16):
            inter = ec.GATED_WIDTHS[dtype][1]
            x = ec.gated_inputs(kind, inter, 5, dtype)
            ec.check_gated(ec.act_fp32(x, None, kind).to(dtype), x, kind)                        # the right answer passes
            g, u = ec.act_operands(x, None, kind)
            keep = torch.ones_like(g, dtype=torch.bool)
            if name == "gate and up columns swapped":
                bad = ec.act_fp32(torch.cat((x[:, inter:], x[:, :inter]), dim=1), None, kind)
            elif name == "erf GELU in place of the tanh form":
                if kind != 2:
                    continue
                bad, keep = torch.nn.functional.gelu(g) * u, g.abs() <= 3.0                      # must show at ordinary gate values
            else:
                if kind != 1:
                    continue
                bad = torch.sigmoid(g) * u
            bad = bad.to(dtype)
            with pytest.raises(AssertionError):
                ec.check_gated(bad, x, kind)
            ratio = ec.gated_ratio(bad, x, kind)[keep]
            assert float(ratio.max()) > 1.0
            scored.append(f"{'SwiGLU' if kind == 1 else 'GeGLU'} {'fp32' if dtype == F32 else 'bf16'}: {float(ratio.max()):.3g} x bound, "
                          f"{float((ratio > 1).float().mean()):.0%} of elements")
    _say(capsys, f"gated, rejected: {name} (" + "; ".join(scored) + ")")
    assert scored


# ---- the argument contract -------------------------------------------------------------------------------------------------------
def _p(v):
    return None if v is None else C.c_void_p(v)


def ln_pieces(lib, a=P, a_bias=None, b=P, gamma=P, beta=P, rows=4, d=256, out=P, pieces=P):
    return lib.ts_add_layernorm_pieces(0, _p(a), _p(a_bias), _p(b), _p(gamma), _p(beta), 1e-12, rows, d, _p(out), _p(pieces), None)


def rms_pieces(lib, a=P, b=P, gamma=P, rows=4, d=256, out_sum=P, out_norm=P, pieces=P):
    return lib.ts_add_rmsnorm_pieces(0, _p(a), _p(b), _p(gamma), 1e-6, rows, d, _p(out_sum), _p(out_norm), _p(pieces), None)


def gemma_pieces(lib, y=P, x=P, w_post=P, w_next=P, rows=4, d=256, out_sum=P, out_norm=P, pieces=P):
    return lib.ts_gemma_norm_pieces(0, _p(y), _p(x), _p(w_post), _p(w_next), 1e-6, rows, d, _p(out_sum), _p(out_norm), _p(pieces), None)


def act_pieces(lib, x=P, bias=None, rows=4, n=256, kind=0, pieces=P):
    return lib.ts_act_pieces(0, _p(x), _p(bias), rows, n, kind, _p(pieces), None)


def attention(lib, qkv=P, qkv_bias=None, mask=None, batch=2, seq=16, hq=4, hkv=2, hd=64, causal=0, scale=0.125, out=P, pieces=None):
    return lib.ts_attention_float(0, _p(qkv), _p(qkv_bias), _p(mask), batch, seq, hq, hkv, hd, causal, scale, _p(out), _p(pieces), None)


def pool(lib, hidden=P, mask=P, n=2, seq=8, d=64, out=P, out_ld=64):
    return lib.ts_pool_normalize(0, _p(hidden), 0, _p(mask), n, seq, d, 0, 1, _p(out), 0, out_ld, None)


def add_ln(lib, a=P, b=P, gamma=P, beta=P, rows=4, d=256, dtype=0, out=P):
    return lib.ts_add_layernorm(0, _p(a), _p(b), _p(gamma), _p(beta), 1e-12, rows, d, dtype, _p(out), None)


def embed_ln(lib, ids=P, type_ids=P, word=P, pos=P, type=P, n_word=100, n_pos=64, n_type=2, gamma=P, beta=P, tokens=32, seq=16, d=256, dtype=0, out=P):
    return lib.ts_embed_layernorm(0, _p(ids), _p(type_ids), _p(word), _p(pos), _p(type), n_word, n_pos, n_type, _p(gamma), _p(beta), 1e-12,
                                  tokens, seq, d, dtype, _p(out), None)


def add_rms(lib, a=P, b=P, gamma=P, rows=4, d=256, dtype=0, out_sum=P, out_norm=P):
    return lib.ts_add_rmsnorm(0, _p(a), _p(b), _p(gamma), 1e-6, rows, d, dtype, _p(out_sum), _p(out_norm), None)


def gemma_norm(lib, y=P, x=P, w_post=P, w_next=P, rows=4, d=256, dtype=0, out_sum=P, out_norm=P):
    return lib.ts_gemma_norm(0, _p(y), _p(x), _p(w_post), _p(w_next), 1e-6, rows, d, dtype, _p(out_sum), _p(out_norm), None)


def attn_short(lib, qkv=P, mask=None, batch=2, seq=16, heads=4, hd=64, out=P):
    return lib.ts_attention_short(0, _p(qkv), _p(mask), batch, seq, heads, hd, _p(out), None)


def attn_gqa(lib, qkv=P, mask=None, batch=2, seq=16, hq=4, hkv=2, hd=128, causal=1, out=P):
    return lib.ts_attention_gqa(0, _p(qkv), _p(mask), batch, seq, hq, hkv, hd, causal, _p(out), None)


def qk_rope(lib, qkv=P, qw=P, kw=P, cos=P, sin=P, tokens=32, seq=16, hq=4, hkv=2, hd=128, dtype=0):
    return lib.ts_qk_norm_rope(0, _p(qkv), _p(qw), _p(kw), _p(cos), _p(sin), 1e-6, tokens, seq, hq, hkv, hd, dtype, None)


def gemma_qk_rope(lib, qkv=P, qw=P, kw=P, cos=P, sin=P, tokens=32, seq=16, hq=4, hkv=2, hd=256, dtype=0):
    return lib.ts_gemma_qk_norm_rope(0, _p(qkv), _p(qw), _p(kw), _p(cos), _p(sin), 1e-6, tokens, seq, hq, hkv, hd, dtype, None)


def swiglu(lib, gate_up=P, rows=4, inter=256, dtype=0, out=P):
    return lib.ts_swiglu(0, _p(gate_up), rows, inter, dtype, _p(out), None)


def geglu(lib, gate_up=P, rows=4, inter=256, dtype=0, out=P):
    return lib.ts_geglu(0, _p(gate_up), rows, inter, dtype, _p(out), None)


def split3(lib, x=P, rows=4, k=256, pattern=0, out=P):
    return lib.ts_split_pieces(0, _p(x), rows, k, pattern, _p(out), None)


PRODUCERS = (ln_pieces, rms_pieces, gemma_pieces, act_pieces)
NORM_PRODUCERS = (ln_pieces, rms_pieces, gemma_pieces)
NORMS = (add_ln, embed_ln, add_rms, gemma_norm)                # the storage-typed entry points of the norm family
# every pointer each of the other entry points refuses as NULL, and every one it wants 16-byte aligned
REQUIRED = {add_ln: ("a", "b", "gamma", "beta", "out"), embed_ln: ("ids", "word", "pos", "type", "gamma", "beta", "out"),
            add_rms: ("a", "gamma", "out_norm"), gemma_norm: ("x", "w_next", "out_norm"), attn_short: ("qkv", "out"),
            attn_gqa: ("qkv", "out"), qk_rope: ("qkv", "qw", "kw", "cos", "sin"), gemma_qk_rope: ("qkv", "qw", "kw", "cos", "sin"),
            swiglu: ("gate_up", "out"), geglu: ("gate_up", "out"), split3: ("x", "out")}
ALIGNED16 = {add_ln: ("a", "b", "gamma", "beta", "out"), embed_ln: ("word", "pos", "type", "gamma", "beta", "out"),
             add_rms: ("a", "b", "gamma", "out_sum", "out_norm"), gemma_norm: ("y", "x", "w_post", "w_next", "out_sum", "out_norm"),
             attn_short: ("qkv", "out"), attn_gqa: ("qkv", "out"), qk_rope: ("qkv", "qw", "kw", "cos", "sin"),
             gemma_qk_rope: ("qkv", "qw", "kw", "cos", "sin"), swiglu: ("gate_up", "out"), geglu: ("gate_up", "out"), split3: ("x",)}
EMPTY = {add_ln: "rows", embed_ln: "tokens", add_rms: "rows", gemma_norm: "rows", attn_short: "batch", attn_gqa: "batch",
         qk_rope: "tokens", gemma_qk_rope: "tokens", swiglu: "rows", geglu: "rows", split3: "rows"}


def test_refusals_come_before_the_device_check():
    lib = _ffi.load()
    inv, uns = ec.TS_ERR_INVALID, ec.TS_ERR_UNSUPPORTED
    for f in PRODUCERS:
        assert f(lib, pieces=None) == inv, f.__name__                                         # NULL pieces
        assert f(lib, pieces=P + 4) == inv, f.__name__                                        # pieces not 8-byte aligned
    assert ln_pieces(lib, a_bias=P + 8) == inv                                                # a bias not 16-byte aligned
    assert act_pieces(lib, bias=P + 8) == inv
    assert attention(lib, qkv_bias=P + 8) == inv
    for f in NORM_PRODUCERS:
        assert f(lib, d=6) == inv and f(lib, d=254) == inv, f.__name__                        # d not a multiple of 4
        assert f(lib, d=1028) == inv, f.__name__                                              # above the fp32 limit of 1024
        assert f(lib, d=0) == inv and f(lib, rows=-1) == inv, f.__name__
    assert act_pieces(lib, n=6) == inv and act_pieces(lib, n=254) == inv and act_pieces(lib, n=0) == inv
    assert act_pieces(lib, kind=3) == inv and act_pieces(lib, kind=-1) == inv
    assert gemma_pieces(lib, w_post=None) == inv                                              # y without w_post
    assert attention(lib, hq=6, hkv=4) == inv                                                 # q_heads % kv_heads != 0
    assert attention(lib, scale=0.0) == inv and attention(lib, scale=float("nan")) == inv and attention(lib, scale=-0.125) == inv
    assert attention(lib, out=None, pieces=None) == inv                                       # nothing to write
    assert attention(lib, out=None, pieces=P + 4) == inv
    assert pool(lib, out_ld=63) == inv                                                        # out_ld < d
    for hd, seq in ((64, 513), (128, 257), (256, 129), (32, 16)):
        assert attention(lib, hd=hd, seq=seq) == uns, (hd, seq)
    assert b"head size" in lib.ts_last_error()
    # nothing to do is not an error (and needs no device)
    for f in PRODUCERS:
        assert f(lib, rows=0) == 0, f.__name__
    assert attention(lib, batch=0) == 0 and pool(lib, n=0) == 0
    # the other entry points: NULL and misaligned pointers, one at a time
    for f, names in REQUIRED.items():
        for name in names:
            assert f(lib, **{name: None}) == inv, (f.__name__, name)
    for f, names in ALIGNED16.items():
        for name in names:
            assert f(lib, **{name: P + 8}) == inv, (f.__name__, name)
    assert split3(lib, out=P + 4) == inv                                                      # out: 8-byte aligned
    assert gemma_norm(lib, w_post=None) == inv                                                # y without w_post
    # storage types
    for f in NORMS + (qk_rope, gemma_qk_rope, swiglu, geglu):
        assert f(lib, dtype=2) == inv and f(lib, dtype=-1) == inv, f.__name__
    assert b"dtype" in lib.ts_last_error()
    # shape limits
    for f in NORMS:
        assert f(lib, d=6) == inv and f(lib, d=1028) == inv and f(lib, d=0) == inv, f.__name__          # fp32: multiples of 4 up to 1024
        assert f(lib, dtype=1, d=4) == inv and f(lib, dtype=1, d=12) == inv and f(lib, dtype=1, d=2056) == inv, f.__name__   # bf16: of 8 up to 2048
        assert f(lib, **{EMPTY[f]: -1}) == inv, f.__name__
    assert b"must be a multiple of 4 and at most 1024" in lib.ts_last_error()
    assert embed_ln(lib, seq=0) == inv and embed_ln(lib, n_word=0) == inv and embed_ln(lib, n_pos=0) == inv and embed_ln(lib, n_type=0) == inv
    for f in (attn_short, attn_gqa):
        assert f(lib, batch=-1) == inv and f(lib, seq=0) == inv, f.__name__
        assert f(lib, seq=129) == uns and f(lib, hd=32) == uns and f(lib, hd=256) == uns, f.__name__
        assert b"at most 128 tokens" in lib.ts_last_error()
    assert attn_short(lib, heads=0) == inv and attn_short(lib, hd=128) == uns
    assert attn_gqa(lib, hq=0) == inv and attn_gqa(lib, hkv=0) == inv and attn_gqa(lib, hq=6, hkv=4) == inv and attn_gqa(lib, hd=64) == uns
    for f, other in ((qk_rope, 256), (gemma_qk_rope, 128)):
        assert f(lib, tokens=-1) == inv and f(lib, seq=0) == inv and f(lib, hq=0) == inv and f(lib, hkv=0) == inv, f.__name__
        assert f(lib, hd=other) == uns and f(lib, hd=64) == uns, f.__name__
        assert b"head size" in lib.ts_last_error()
    for f in (swiglu, geglu):
        assert f(lib, inter=6) == inv and f(lib, inter=0) == inv and f(lib, dtype=1, inter=12) == inv and f(lib, rows=-1) == inv, f.__name__
    assert split3(lib, k=6) == inv and split3(lib, k=0) == inv and split3(lib, pattern=2) == inv and split3(lib, pattern=-1) == inv
    assert split3(lib, rows=-1) == inv
    # the empty call
    for f, name in EMPTY.items():
        assert f(lib, **{name: 0}) == 0, f.__name__


def test_rotary_and_gated_refusals_at_their_edges():
    """What the loop above leaves out for ts_qk_norm_rope / ts_gemma_qk_norm_rope / ts_swiglu / ts_geglu: both storage types, the
    widths on either side of one 16-byte access, negative counts, every misalignment of every pointer, and the empty call with
    everything else in order - all without a device."""
    lib = _ffi.load()
    inv, uns = ec.TS_ERR_INVALID, ec.TS_ERR_UNSUPPORTED
    for f in (swiglu, geglu):
        for dtype, vec in ((0, 4), (1, 8)):
            for inter in (vec - 1, vec // 2, 1, 0, -vec, vec + 1, 2 * vec - 1, 31 * vec + vec // 2, 3072 + vec // 2):
                assert f(lib, dtype=dtype, inter=inter) == inv, (f.__name__, dtype, inter)
            assert b"must be a multiple of %d" % vec in lib.ts_last_error()
            assert f(lib, dtype=dtype, inter=vec, rows=-1) == inv, (f.__name__, dtype)
            assert f(lib, dtype=dtype, inter=vec, rows=0) == 0 and f(lib, dtype=dtype, inter=3072, rows=0) == 0, (f.__name__, dtype)
            for name in ALIGNED16[f]:
                for off in (1, 2, 4, 8, 12):
                    assert f(lib, dtype=dtype, inter=vec, **{name: P + off}) == inv, (f.__name__, dtype, name, off)
            assert b"16-byte aligned" in lib.ts_last_error()
        assert f(lib, dtype=1, inter=4) == inv                                                  # one fp32 access is half a bf16 one
    for f, own, other in ((qk_rope, 128, 256), (gemma_qk_rope, 256, 128)):
        for dtype in (0, 1):
            for seq in (0, -1, -16):
                assert f(lib, dtype=dtype, seq=seq) == inv, (f.__name__, dtype, seq)
            for heads in (0, -1):
                assert f(lib, dtype=dtype, hq=heads) == inv and f(lib, dtype=dtype, hkv=heads) == inv, (f.__name__, dtype, heads)
                assert f(lib, dtype=dtype, hq=heads, hkv=heads) == inv, (f.__name__, dtype, heads)
            assert f(lib, dtype=dtype, tokens=-1) == inv, (f.__name__, dtype)
            for hd in (other, 64, 0, -own, own + 8, 4 * own):
                assert f(lib, dtype=dtype, hd=hd) == uns, (f.__name__, dtype, hd)
                assert b"head size %d: this kernel serves head size %d" % (hd, own) in lib.ts_last_error()
            for name in ALIGNED16[f]:
                for off in (1, 2, 4, 8, 12):
                    assert f(lib, dtype=dtype, **{name: P + off}) == inv, (f.__name__, dtype, name, off)
            assert b"16-byte aligned" in lib.ts_last_error()
            # nothing to do: OK whatever the other counts are, as long as they are valid ...
            assert f(lib, dtype=dtype, tokens=0) == 0 and f(lib, dtype=dtype, tokens=0, seq=1, hq=1, hkv=1) == 0, (f.__name__, dtype)
            # ... and a refusal still comes first
            assert f(lib, dtype=dtype, tokens=0, seq=0) == inv and f(lib, dtype=dtype, tokens=0, hd=other) == uns, (f.__name__, dtype)
            assert f(lib, dtype=dtype, tokens=0, qkv=P + 8) == inv and f(lib, dtype=dtype, tokens=0, cos=None) == inv, (f.__name__, dtype)
    for f in (swiglu, geglu):
        assert f(lib, rows=0, inter=6) == inv and f(lib, rows=0, out=P + 8) == inv and f(lib, rows=0, gate_up=None) == inv, f.__name__


@pytest.mark.skipif(gpu_available(), reason="fake pointers: only where the device check refuses the call")
def test_valid_arguments_reach_the_device_check():
    """The same calls with nothing to refuse: TS_ERR_NODEVICE, so the refusals above were about the argument they changed."""
    lib = _ffi.load()
    nod = ec.TS_ERR_NODEVICE
    for f in PRODUCERS + (attention, pool):
        assert f(lib) == nod, f.__name__
    assert ln_pieces(lib, a_bias=P, d=1024) == nod and rms_pieces(lib, b=None, out_sum=None, d=4) == nod
    assert gemma_pieces(lib, y=None, w_post=None, out_sum=None) == nod
    assert act_pieces(lib, bias=P, kind=2, pieces=P + 8) == nod
    assert attention(lib, qkv_bias=P, mask=P, out=None, pieces=P + 8, causal=1) == nod
    for hd, seq in ((64, 512), (128, 256), (256, 128)):
        assert attention(lib, hd=hd, seq=seq) == nod, (hd, seq)
    assert pool(lib, out_ld=72) == nod
    for f in REQUIRED:
        assert f(lib) == nod, f.__name__
    for f in NORMS:
        assert f(lib, d=4) == nod and f(lib, d=1024) == nod and f(lib, dtype=1, d=8) == nod and f(lib, dtype=1, d=2048) == nod, f.__name__
    assert embed_ln(lib, type_ids=None) == nod and add_rms(lib, b=None, out_sum=None) == nod
    assert gemma_norm(lib, y=None, w_post=None, out_sum=None) == nod
    for seq in (1, 64, 65, 128):
        assert attn_short(lib, seq=seq, mask=P) == nod and attn_gqa(lib, seq=seq, mask=P, causal=0) == nod, seq
    assert attn_gqa(lib, seq=128, hq=3, hkv=1) == nod and attn_gqa(lib, seq=128, hq=8, hkv=2) == nod
    assert qk_rope(lib, dtype=1) == nod and gemma_qk_rope(lib, dtype=1) == nod
    assert swiglu(lib, dtype=1, inter=8) == nod and geglu(lib, inter=4) == nod
    assert split3(lib, pattern=1, out=P + 8, k=4) == nod


@pytest.mark.skipif(gpu_available(), reason="fake pointers: only where the device check refuses the call")
def test_the_fused_forwards_named_limits_are_the_librarys_refusal_boundaries():
    """fused_forward.py decides by these names whether a model or a batch takes a kernel; the library holds the limits themselves
    (csrc/encoder_plan.h).  At each named limit a call gets as far as the device check; one step past it, it is refused."""
    from theoremsearch_amd import fused_forward as ff
    lib = _ffi.load()
    nod, refused = ec.TS_ERR_NODEVICE, (ec.TS_ERR_INVALID, ec.TS_ERR_UNSUPPORTED)
    assert attn_short(lib, hd=ff._SHORT_HEAD, seq=ff._SHORT_MAX_SEQ) == nod
    assert attn_short(lib, hd=ff._SHORT_HEAD, seq=ff._SHORT_MAX_SEQ + 1) in refused and attn_short(lib, hd=ff._SHORT_HEAD + 1, seq=ff._SHORT_MAX_SEQ) in refused
    assert attn_gqa(lib, hd=ff._GQA_HEAD, seq=ff._GQA_MAX_SEQ) == nod
    assert attn_gqa(lib, hd=ff._GQA_HEAD, seq=ff._GQA_MAX_SEQ + 1) in refused and attn_gqa(lib, hd=ff._GQA_HEAD + 1, seq=ff._GQA_MAX_SEQ) in refused
    for hd, seq in ff._FLOAT_ATTENTION_MAX_SEQ.items():
        assert attention(lib, hd=hd, seq=seq) == nod and attention(lib, hd=hd, seq=seq + 1) in refused, (hd, seq)
    assert attention(lib, hd=max(ff._FLOAT_ATTENTION_MAX_SEQ) * 2) in refused
    for dtype, vec in ((0, 4), (1, 8)):
        for f in NORMS:
            assert f(lib, dtype=dtype, d=ff._NORM_MAX_VECS * vec) == nod, (f.__name__, dtype)
            assert f(lib, dtype=dtype, d=(ff._NORM_MAX_VECS + 1) * vec) in refused, (f.__name__, dtype)
