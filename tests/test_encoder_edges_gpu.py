"""Edge shapes of the encoder's kernels around the GEMMs, each against fp64 on the same inputs (tests/encoder_common.py):
* the one-wave-per-row norm kernels (ts_add_layernorm, ts_add_rmsnorm, ts_gemma_norm, ts_embed_layernorm) at every access class
  (1, 2 or 4 16-byte accesses per lane) and both edges of each, fp32 and bf16, with 1, 5 and 259 rows;
* ts_attention_float next to every 16-token tile edge up to the longest sequence of each head size, causal and not, under
  right / left padding, holes, a sequence with a single key and one with none - a query row without an allowed key is zeros,
  in the context and in the pieces;
* ts_pool_normalize under left padding, holes and a row without a token, into a padded output (out_ld > d) and from a
  misaligned `hidden` (the general kernel on an encoder-shaped input), n = 1.
Every output the tests allocate lies in a sentinel-filled buffer whose margins must come back untouched."""
import ctypes as C

import pytest
import torch

import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 1}
WIDTHS = {F32: ec.NORM_WIDTHS_F32, BF16: ec.NORM_WIDTHS_BF16}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- norm width classes ----------------------------------------------------------------------------------------------------------
def tally(share, name, have, ref):
    """Add the elements of `have` that differ from the module's `ref` to the count kept for the compared tensor `name`."""
    diff, count = share.get(name, (0, 0))
    share[name] = (diff + int((have != ref).sum()), count + have.numel())


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_add_layernorm_at_every_width_class(dtype, capsys):
    lib = _ffi.load()
    worst = 0.0
    for d in WIDTHS[dtype]:
        for rows in ec.NORM_ROWS:
            a, _, b, gamma, beta = (t.cuda() for t in ec.layernorm_inputs(d, rows, dtype))
            out = ec.guarded((rows, d), dtype)
            _ffi.check(lib.ts_add_layernorm(0, P(a), P(b), P(gamma), P(beta), ec.LN_EPS, rows, d, CODE[dtype], P(out), stream()))
            torch.cuda.synchronize()
            r = ec.norm_ratio(out, ec.layernorm_ref(a, None, b, gamma, beta), ec.NORM_TOL[dtype])
            assert r <= 1.0, (dtype, d, rows, r)
            assert torch.equal(out[0], beta), (dtype, d, rows, "the all-zero row is beta")
            ec.assert_margins(out)
            worst = max(worst, r)
    with capsys.disabled():
        print(f"\nts_add_layernorm {dtype}: worst error / tolerance = {worst:.4f}", end="")


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_embed_layernorm_at_every_width_class(dtype, capsys):
    """Token counts 1, 5 and 259 (the last workgroup holds 1 or 3 waves), a sequence length that does not divide them, ids at
    both ends of each table, token types given and absent."""
    lib = _ffi.load()
    worst = 0.0
    V, T, S = 50, 2, 7
    for d in WIDTHS[dtype]:
        g = torch.Generator(device="cpu").manual_seed(900 + d)
        word, pos, typ = (torch.randn((n, d), generator=g).to(dtype).cuda() for n in (V, S, T))
        gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).to(dtype).cuda()
        beta = (0.1 * torch.randn(d, generator=g)).to(dtype).cuda()
        for tokens in ec.NORM_ROWS:
            ids = torch.randint(0, V, (tokens,), generator=g)
            tt = torch.randint(0, T, (tokens,), generator=g)
            ids[0], tt[0] = V - 1, T - 1
            if tokens > 1:
                ids[1], tt[1] = 0, 0
            ids, tt = ids.cuda(), tt.cuda()
            for types in (None, tt):
                out = ec.guarded((tokens, d), dtype)
                _ffi.check(lib.ts_embed_layernorm(0, P(ids), P(types), P(word), P(pos), P(typ), V, S, T, P(gamma), P(beta), ec.LN_EPS,
                                                  tokens, S, d, CODE[dtype], P(out), stream()))
                torch.cuda.synchronize()
                r = ec.norm_ratio(out, ec.embed_layernorm_ref(ids, types, word, pos, typ, gamma, beta, S), ec.NORM_TOL[dtype])
                assert r <= 1.0, (dtype, d, tokens, types is not None, r)
                ec.assert_margins(out)
                worst = max(worst, r)
    with capsys.disabled():
        print(f"\nts_embed_layernorm {dtype}: worst error / tolerance = {worst:.4f}", end="")


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_add_rmsnorm_at_every_width_class(dtype, capsys):
    """Against fp64 on the rounded sum; out_sum is torch's own a + b in the storage type, exactly.  bf16 also follows Qwen3RMSNorm's
    roundings step by step: within one bf16 ulp of the module's own output, and different from it on less than 1e-3 of the
    elements - the caps of test_add_rmsnorm_kernel_matches_the_module_chain, held by each compared tensor on its own (the output
    with the addend, the output without it), counted per width over its three row counts only (one row of d = 8 cannot carry a
    share)."""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    lib = _ffi.load()
    worst = 0.0
    for d in WIDTHS[dtype]:
        share = {}                                                # compared tensor -> [differing elements, elements]
        for rows in ec.NORM_ROWS:
            a, b, gamma = (t.cuda() for t in ec.rmsnorm_inputs(d, rows, dtype))
            norm = Qwen3RMSNorm(d, eps=ec.RMS_EPS).to("cuda", dtype=dtype)
            with torch.no_grad():
                norm.weight.copy_(gamma)
            for bb in (b, None):
                s_ref, want = ec.rmsnorm_ref(a, bb, gamma)
                osum, out = ec.guarded((rows, d), dtype), ec.guarded((rows, d), dtype)
                _ffi.check(lib.ts_add_rmsnorm(0, P(a), P(bb), P(gamma), ec.RMS_EPS, rows, d, CODE[dtype], P(osum), P(out), stream()))
                torch.cuda.synchronize()
                assert torch.equal(osum, s_ref), (dtype, d, rows, bb is not None, "out_sum")
                r = ec.norm_ratio(out, want, ec.NORM_TOL[dtype])
                assert r <= 1.0, (dtype, d, rows, bb is not None, r)
                assert not out[0].any(), (dtype, d, rows, "the all-zero row")
                ec.assert_margins(osum, out)
                worst = max(worst, r)
                if dtype == BF16:
                    with torch.no_grad():
                        module = norm(s_ref)
                    assert (out.float() - module.float()).abs().max().item() <= 2 ** -6 * module.float().abs().max().item(), (d, rows)
                    tally(share, "out with b" if bb is not None else "out without b", out, module)
        for name, (diff, count) in share.items():
            assert diff / count < 1e-3, (d, name, diff, count)
    with capsys.disabled():
        print(f"\nts_add_rmsnorm {dtype}: worst error / tolerance = {worst:.4f}", end="")


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_gemma_norm_at_every_width_class(dtype, capsys):
    """out_sum and out_norm against fp64, with y and without.  bf16 also follows Gemma3RMSNorm's roundings (the residual add in
    the storage type, each norm rounded once): within 2^-6 max(1, |want|) of the modules' own chain and different from it on less
    than 2e-3 of the elements - the caps of test_gemma3_kernels_match_the_modules, held by each compared tensor on its own (out_sum
    and out_norm with y, out_norm without y; out_sum without y is x itself, asserted exactly and not counted), counted per width
    over its three row counts only."""
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm
    lib = _ffi.load()
    worst = 0.0
    tol = ec.NORM_TOL[dtype]
    for d in WIDTHS[dtype]:
        share = {}
        for rows in ec.NORM_ROWS:
            y, x, w_post, w_next = (t.cuda() for t in ec.gemma_inputs(d, rows, dtype))
            post, nxt = (Gemma3RMSNorm(d, eps=ec.RMS_EPS).to("cuda", dtype=dtype) for _ in range(2))
            with torch.no_grad():
                post.weight.copy_(w_post)
                nxt.weight.copy_(w_next)
            for yy, wp in ((y, w_post), (None, None)):
                s_ref, want = ec.gemma_ref(yy, x, wp, w_next)
                osum, out = ec.guarded((rows, d), dtype), ec.guarded((rows, d), dtype)
                _ffi.check(lib.ts_gemma_norm(0, P(yy), P(x), P(wp), P(w_next), ec.RMS_EPS, rows, d, CODE[dtype], P(osum), P(out), stream()))
                torch.cuda.synchronize()
                rs, r = ec.norm_ratio(osum, s_ref, tol), ec.norm_ratio(out, want, tol)
                assert rs <= 1.0 and r <= 1.0, (dtype, d, rows, yy is not None, rs, r)
                assert not out[0].any() and not osum[0].any(), (dtype, d, rows, "the all-zero row")
                if yy is None:
                    assert torch.equal(osum, x)
                ec.assert_margins(osum, out)
                worst = max(worst, rs, r)
                if dtype == BF16:
                    with torch.no_grad():
                        m_sum = x if yy is None else x + post(yy)
                        m_out = nxt(m_sum)
                    compared = (("out_sum with y", osum, m_sum), ("out with y", out, m_out)) if yy is not None else (("out without y", out, m_out),)
                    for name, have, ref in compared:
                        assert (have.float() - ref.float()).abs().max().item() <= 2 ** -6 * max(1.0, ref.float().abs().max().item()), (d, rows, name)
                        tally(share, name, have, ref)
        for name, (diff, count) in share.items():
            assert diff / count < 2e-3, (d, name, diff, count)
    with capsys.disabled():
        print(f"\nts_gemma_norm {dtype}: worst error / tolerance = {worst:.4f}", end="")


# ---- ts_attention_float ------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = ((12, 12, 64), (6, 2, 64), (16, 8, 128), (4, 4, 128), (3, 1, 256))
ATTN_LENGTHS = (1, 15, 16, 17, 31, 47, 63, 64, 65, 127, 128)
ATTN_MORE = {64: (129, 255, 257, 511, 512), 128: (255, 256), 256: ()}


def guarded_split(x):
    rows, k = x.shape
    out = ec.guarded((rows, 3 * k), BF16, align=8)
    _ffi.check(_ffi.load().ts_split_pieces(0, P(x), rows, k, 0, P(out), stream()))
    return out


@pytest.mark.parametrize("hq,hkv,hd", ATTN_SHAPES, ids=lambda v: str(v))
def test_float_attention_at_the_tile_edges_under_every_mask(hq, hkv, hd, capsys):
    """Through fused_forward.attention_float against fp64 (err < 2e-5 on N(0, 1.5^2) inputs, the bound of
    test_float_attention_kernel_matches_fp64): B = 3, every length next to a 16-token tile edge, causal and not, one mask of each
    kind per (shape, length) from a seeded generator.  Every row with an allowed key is compared; rows without one - left-padded
    rows under causal, rows in front of a single key, the keyless sequence - are exactly zero in the context and in the pieces;
    the pieces are ts_split_pieces of the context.  attention_float allocates its own outputs, so every case is repeated as a direct
    call into guarded buffers, which must hold the same bits."""
    from theoremsearch_amd.fused_forward import attention_float
    lib = _ffi.load()
    B, scale = 3, hd ** -0.5
    g = torch.Generator(device="cpu").manual_seed(1000 * hq + 10 * hkv + hd)
    worst, zero_rows = 0.0, 0
    for S in ATTN_LENGTHS + ATTN_MORE[hd]:
        qkv = (torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g) * 1.5).cuda()
        masks = ec.attention_masks(B, S, g)
        assert tuple(masks) == ec.ATTN_MASK_KINDS
        for kind, mask in masks.items():
            mask = None if mask is None else mask.cuda()
            for causal in (False, True):
                tag = (hq, hkv, hd, S, kind, causal)
                want, has_key = ec.attention_ref(qkv, mask, hq, hkv, hd, causal, scale)
                got, pieces = attention_float(qkv, mask, B, S, hq, hkv, hd, causal, scale, want_pieces=True)
                sp = guarded_split(got.view(B * S, -1))
                # the same call straight into guarded buffers: the same bits, nothing written outside them
                g_out, g_pieces = ec.guarded((B, S, hq * hd), F32), ec.guarded((B * S, 3 * hq * hd), BF16, align=8)
                _ffi.check(lib.ts_attention_float(0, P(qkv), None, P(mask), B, S, hq, hkv, hd, 1 if causal else 0, scale, P(g_out), P(g_pieces),
                                                  stream()))
                torch.cuda.synchronize()
                assert ec.same_bits(g_out, got) and ec.same_bits(g_pieces, pieces), (tag, "direct call into guarded buffers")
                ec.assert_margins(g_out, g_pieces)
                assert torch.isfinite(got).all(), tag
                if has_key.any():
                    err = (got.double() - want)[has_key].abs().max().item()
                    assert err < 2e-5, (tag, err)
                    worst = max(worst, err)
                if not has_key.all():
                    assert not got[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
                    assert not pieces.view(B, S, -1)[~has_key].any(), (tag, "... in the pieces too")
                    zero_rows += int((~has_key).sum())
                assert ec.same_bits(pieces, sp), (tag, "pieces differ from ts_split_pieces(context)")
                ec.assert_margins(sp)
                if kind == "keyless":
                    assert not has_key[B - 1].any()
    assert zero_rows > 0
    with capsys.disabled():
        print(f"\nts_attention_float {hq}/{hkv} x {hd}: worst error {worst / 2e-5:.3f} of 2e-5, {zero_rows} keyless rows exactly zero", end="")


@pytest.mark.parametrize("hq,hkv,hd", ((6, 2, 64), (4, 4, 128), (3, 1, 256)), ids=lambda v: str(v))
def test_float_attention_pieces_only_bias_and_guarded_outputs(hq, hkv, hd):
    """Per head size: the pieces without the context are the pieces with it; the stacked projection's bias added on the way in
    gives the answer on qkv + bias (the existing 1e-5); a direct call into guarded buffers writes nothing outside them."""
    from theoremsearch_amd.fused_forward import attention_float
    lib = _ffi.load()
    B, scale = 3, hd ** -0.5
    g = torch.Generator(device="cpu").manual_seed(7000 + hd)
    for S in (17, max(ATTN_LENGTHS + ATTN_MORE[hd])):                      # a ragged tile and the head size's longest sequence
        qkv = (torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g) * 1.5).cuda()
        mask = ec.attention_masks(B, S, g)["left"].cuda()
        for causal in (False, True):
            ctx, both = attention_float(qkv, mask, B, S, hq, hkv, hd, causal, scale, want_pieces=True)
            none, only = attention_float(qkv, mask, B, S, hq, hkv, hd, causal, scale, want_pieces=True, want_context=False)
            sp = guarded_split(ctx.view(B * S, -1))
            torch.cuda.synchronize()
            assert none is None and ec.same_bits(only, both) and ec.same_bits(both, sp), (hd, S, causal)
            out, pieces = ec.guarded((B, S, hq * hd), F32), ec.guarded((B * S, 3 * hq * hd), BF16, align=8)
            _ffi.check(lib.ts_attention_float(0, P(qkv), None, P(mask), B, S, hq, hkv, hd, 1 if causal else 0, scale, P(out), P(pieces), stream()))
            only_p = ec.guarded((B * S, 3 * hq * hd), BF16, align=8)
            _ffi.check(lib.ts_attention_float(0, P(qkv), None, P(mask), B, S, hq, hkv, hd, 1 if causal else 0, scale, None, P(only_p), stream()))
            torch.cuda.synchronize()
            assert ec.same_bits(out, ctx) and ec.same_bits(pieces, both) and ec.same_bits(only_p, both), (hd, S, causal)
            ec.assert_margins(out, pieces, only_p, sp)
            # the bias of the GEMM in front, added on the way in
            qb = torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g).cuda()
            bias = torch.randn((hq + 2 * hkv) * hd, generator=g).cuda()
            want = attention_float(qb + bias, mask, B, S, hq, hkv, hd, causal, scale)[0]
            got, gp = attention_float(qb, mask, B, S, hq, hkv, hd, causal, scale, want_pieces=True, bias=bias)
            ref, has_key = ec.attention_ref(qb, mask, hq, hkv, hd, causal, scale, bias=bias)
            sp = guarded_split(got.view(B * S, -1))
            torch.cuda.synchronize()
            assert (got - want).abs().max().item() < 1e-5, (hd, S, causal)
            assert (got.double() - ref)[has_key].abs().max().item() < 2e-5 and not got[~has_key].any(), (hd, S, causal)
            assert ec.same_bits(gp, sp), (hd, S, causal)


# ---- ts_pool_normalize -------------------------------------------------------------------------------------------------------------
def _pool(lib, hidden, mask, pooling, normalize, out, out_ld):
    n, S, d = hidden.shape
    _ffi.check(lib.ts_pool_normalize(0, P(hidden), CODE[hidden.dtype], P(mask), n, S, d, pooling, normalize, P(out), CODE[out.dtype], out_ld, stream()))


def _misaligned(t):
    """The same values at an address one element past a 16-byte boundary: the general kernel takes them."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("dtype", (F32, BF16), ids=("f32", "bf16"))
def test_pool_normalize_masks_layouts_and_the_general_kernel(dtype, capsys):
    """fp32 / bf16 hidden states into fp32 and bf16 outputs at the tolerances of test_fused_pooling_epilogue_matches_torch: left
    padding and holes (the last kept token of a holed row is not the last position) under all three poolings, a row without a token under MEAN (zeros, normalised or not); out_ld = d + 8 into a
    sentinel-filled buffer (the extra columns stay untouched); `hidden` one element off a 16-byte boundary; n = 1."""
    lib = _ffi.load()
    worst = 0.0
    for d in (8, 100, 768, 1024):
        for S in (1, 19, 1100):
            for n in ((5, 1) if (d, S) == (768, 19) else (5,)):
                g = torch.Generator(device="cpu").manual_seed(31 * d + S)
                hidden = torch.randn((n, S, d), generator=g).to(dtype).cuda()
                off = _misaligned(hidden)
                left, holes = (m.cuda() for m in ec.pool_masks(n, S, d))
                empty = holes.clone()
                empty[n // 2] = 0                                                   # a row without a token
                for mask, poolings in ((left, (0, 1, 2)), (holes, (0, 1, 2)), (empty, (0,))):
                    for pooling in poolings:
                        for normalize in (0, 1):
                            want = ec.pool_ref(hidden, mask, pooling, bool(normalize))
                            if mask is empty:
                                assert not want[n // 2].any()
                            for out_dtype, rtol in ((F32, 1e-5), (BF16, 2 ** -7)):
                                for src, ld in ((hidden, d), (hidden, d + 8), (off, d)):
                                    tag = (dtype, d, S, n, pooling, normalize, out_dtype, ld, src is off)
                                    out = ec.guarded((n, ld), out_dtype)
                                    _pool(lib, src, mask, pooling, normalize, out, ld)
                                    torch.cuda.synchronize()
                                    got = out[:, :d].double()
                                    err = (got - want).abs()
                                    assert torch.isfinite(got).all() and bool((err <= 1e-5 + rtol * want.abs()).all()), (tag, err.max().item())
                                    if mask is empty:
                                        assert not out[n // 2, :d].any(), (tag, "a row without a token: zeros")
                                    assert ld == d or ec.untouched(out[:, d:]), (tag, "columns past d were written")
                                    ec.assert_margins(out)
                                    if out_dtype == F32:
                                        worst = max(worst, float((err / (1e-5 + rtol * want.abs())).max()))
    with capsys.disabled():
        print(f"\nts_pool_normalize {dtype} in, fp32 out: worst error / (1e-5 + 1e-5 |want|) = {worst:.3f}", end="")
