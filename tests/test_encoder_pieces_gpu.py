"""The four producers that write bf16 pieces themselves - ts_add_layernorm_pieces, ts_add_rmsnorm_pieces, ts_gemma_norm_pieces,
ts_act_pieces - called directly, at every access class of the one-wave-per-row kernels and both edges of each, with 1, 5 and
259 rows (the last workgroup holds 1 or 3 waves), an all-zero row, every optional argument given and absent, in place, and
past the elementwise kernels' grid cap.  References, bounds and inputs: tests/encoder_common.py (checked without a GPU in
tests/test_encoder_ref_cpu.py).  Every output lies in a sentinel-filled buffer whose margins must come back untouched."""
import ctypes as C

import pytest
import torch

import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def split_pieces(x):
    """ts_split_pieces(x, pattern 0) into a guarded buffer."""
    rows, k = x.shape
    out = ec.guarded((rows, 3 * k), BF16, align=8)
    _ffi.check(_ffi.load().ts_split_pieces(0, P(x), rows, k, 0, P(out), stream()))
    return out


def check_out_and_pieces(out, pieces, plain, want64, tag):
    """The producer's fp32 output equals the plain entry's bit for bit and fp64 within 2e-5; its pieces equal ts_split_pieces of
    the output and split_ref of it, bit for bit.  Returns the worst error / tolerance."""
    torch.cuda.synchronize()
    assert ec.same_bits(out, plain), (tag, "fp32 output differs from the plain entry's")
    sp = split_pieces(out)
    torch.cuda.synchronize()
    assert ec.same_bits(pieces, sp), (tag, "pieces differ from ts_split_pieces(out, 0)")
    ec.assert_margins(sp)
    return ec.check_norm_pieces(out, pieces, want64)


def test_add_layernorm_pieces_at_every_width_class(capsys):
    lib = _ffi.load()
    worst = 0.0
    for d in ec.NORM_WIDTHS_F32:
        for rows in ec.NORM_ROWS:
            a, a_bias, b, gamma, beta = (t.cuda() for t in ec.layernorm_inputs(d, rows))
            for ab in (None, a_bias):
                tag = (d, rows, ab is not None)
                out, pieces, plain = ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8), ec.guarded((rows, d), F32)
                _ffi.check(lib.ts_add_layernorm_pieces(0, P(a), P(ab), P(b), P(gamma), P(beta), ec.LN_EPS, rows, d, P(out), P(pieces), stream()))
                a_plain = a if ab is None else a + ab                                   # torch's fp32 sum: what the kernel forms
                _ffi.check(lib.ts_add_layernorm(0, P(a_plain), P(b), P(gamma), P(beta), ec.LN_EPS, rows, d, 0, P(plain), stream()))
                worst = max(worst, check_out_and_pieces(out, pieces, plain, ec.layernorm_ref(a, ab, b, gamma, beta), tag))
                if ab is None:                                                          # the all-zero row: exactly beta
                    assert torch.equal(out[0], beta), tag
                    assert ec.same_bits(pieces[0:1], ec.split_ref(beta[None])), tag
                # in place over `a`: the same bits
                a2, pieces2 = ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8)
                a2.copy_(a)
                _ffi.check(lib.ts_add_layernorm_pieces(0, P(a2), P(ab), P(b), P(gamma), P(beta), ec.LN_EPS, rows, d, P(a2), P(pieces2), stream()))
                torch.cuda.synchronize()
                assert ec.same_bits(a2, out) and ec.same_bits(pieces2, pieces), (tag, "in place")
                ec.assert_margins(out, pieces, plain, a2, pieces2)
    with capsys.disabled():
        print(f"\nts_add_layernorm_pieces: worst error / (2e-5 + 2e-5 |want|) = {worst:.4f}", end="")


def test_add_rmsnorm_pieces_at_every_width_class(capsys):
    lib = _ffi.load()
    worst = 0.0
    for d in ec.NORM_WIDTHS_F32:
        for rows in ec.NORM_ROWS:
            a, b, gamma = (t.cuda() for t in ec.rmsnorm_inputs(d, rows))
            for bb in (b, None):
                s_ref, want = ec.rmsnorm_ref(a, bb, gamma)
                for want_sum in (True, False):
                    tag = (d, rows, bb is not None, want_sum)
                    out, pieces, plain = ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8), ec.guarded((rows, d), F32)
                    osum = ec.guarded((rows, d), F32) if want_sum else None
                    psum = ec.guarded((rows, d), F32) if want_sum else None
                    _ffi.check(lib.ts_add_rmsnorm_pieces(0, P(a), P(bb), P(gamma), ec.RMS_EPS, rows, d, P(osum), P(out), P(pieces), stream()))
                    _ffi.check(lib.ts_add_rmsnorm(0, P(a), P(bb), P(gamma), ec.RMS_EPS, rows, d, 0, P(psum), P(plain), stream()))
                    worst = max(worst, check_out_and_pieces(out, pieces, plain, want, tag))
                    assert not out[0].any() and not pieces[0].any(), (tag, "the all-zero row")
                    if want_sum:
                        assert ec.same_bits(osum, psum) and torch.equal(osum, s_ref), (tag, "out_sum")      # a + b in fp32: exact
                        # the residual in place over `a`: the same bits
                        a2, out2, pieces2 = ec.guarded((rows, d), F32), ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8)
                        a2.copy_(a)
                        _ffi.check(lib.ts_add_rmsnorm_pieces(0, P(a2), P(bb), P(gamma), ec.RMS_EPS, rows, d, P(a2), P(out2), P(pieces2), stream()))
                        torch.cuda.synchronize()
                        assert ec.same_bits(a2, osum) and ec.same_bits(out2, out) and ec.same_bits(pieces2, pieces), (tag, "in place")
                        ec.assert_margins(osum, psum, a2, out2, pieces2)
                    ec.assert_margins(out, pieces, plain)
    with capsys.disabled():
        print(f"\nts_add_rmsnorm_pieces: worst error / (2e-5 + 2e-5 |want|) = {worst:.4f}", end="")


def test_gemma_norm_pieces_at_every_width_class(capsys):
    lib = _ffi.load()
    worst = 0.0
    tol = ec.NORM_TOL[F32]
    for d in ec.NORM_WIDTHS_F32:
        for rows in ec.NORM_ROWS:
            y, x, w_post, w_next = (t.cuda() for t in ec.gemma_inputs(d, rows))
            for yy, wp in ((y, w_post), (None, None)):
                s_ref, want = ec.gemma_ref(yy, x, wp, w_next)
                for want_sum in (True, False):
                    tag = (d, rows, yy is not None, want_sum)
                    out, pieces, plain = ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8), ec.guarded((rows, d), F32)
                    osum = ec.guarded((rows, d), F32) if want_sum else None
                    psum = ec.guarded((rows, d), F32) if want_sum else None
                    _ffi.check(lib.ts_gemma_norm_pieces(0, P(yy), P(x), P(wp), P(w_next), ec.RMS_EPS, rows, d, P(osum), P(out), P(pieces), stream()))
                    _ffi.check(lib.ts_gemma_norm(0, P(yy), P(x), P(wp), P(w_next), ec.RMS_EPS, rows, d, 0, P(psum), P(plain), stream()))
                    worst = max(worst, check_out_and_pieces(out, pieces, plain, want, tag))
                    assert not out[0].any() and not pieces[0].any(), (tag, "the all-zero row")
                    if want_sum:
                        assert ec.same_bits(osum, psum), (tag, "out_sum")
                        r = ec.norm_ratio(osum, s_ref, tol)
                        assert r <= 1.0, (tag, "out_sum against fp64", r)
                        worst = max(worst, r)
                        if yy is None:
                            assert torch.equal(osum, x), tag                                 # s = x
                        # the residual in place over `x`: the same bits
                        x2, out2, pieces2 = ec.guarded((rows, d), F32), ec.guarded((rows, d), F32), ec.guarded((rows, 3 * d), BF16, align=8)
                        x2.copy_(x)
                        _ffi.check(lib.ts_gemma_norm_pieces(0, P(yy), P(x2), P(wp), P(w_next), ec.RMS_EPS, rows, d, P(x2), P(out2), P(pieces2), stream()))
                        torch.cuda.synchronize()
                        assert ec.same_bits(x2, osum) and ec.same_bits(out2, out) and ec.same_bits(pieces2, pieces), (tag, "in place")
                        ec.assert_margins(osum, psum, x2, out2, pieces2)
                    ec.assert_margins(out, pieces, plain)
    with capsys.disabled():
        print(f"\nts_gemma_norm_pieces: worst error / (2e-5 + 2e-5 |want|) = {worst:.4f}", end="")


@pytest.mark.parametrize("kind", ec.ACT_KINDS)
def test_act_pieces_against_fp64_on_every_element(kind, capsys):
    """No fp32 output exists: the third block equals the first, hi + lo is within pieces_bound of the fp64 activation of the fp32
    operands on every element, hi alone within one bf16 rounding (encoder_common.check_act_pieces)."""
    lib = _ffi.load()
    worst = {"pieces": 0.0, "hi": 0.0}
    for n in ec.ACT_WIDTHS:
        for rows in ec.ACT_ROWS:
            x, bias = (t.cuda() for t in ec.act_inputs(kind, n, rows))
            for b in (None, bias):
                pieces = ec.guarded((rows, 3 * n), BF16, align=8)
                _ffi.check(lib.ts_act_pieces(0, P(x), P(b), rows, n, kind, P(pieces), stream()))
                torch.cuda.synchronize()
                ec.assert_margins(pieces)
                try:
                    r = ec.check_act_pieces(pieces, x, b, kind)
                except AssertionError as e:
                    raise AssertionError(f"kind {kind}, n {n}, rows {rows}, bias {b is not None}: {e}") from None
                worst = {k: max(worst[k], r[k]) for k in worst}
    with capsys.disabled():
        print(f"\nts_act_pieces kind {kind}: worst error / pieces_bound = {worst['pieces']:.3f}, hi alone / its bound = {worst['hi']:.3f}", end="")


def test_elementwise_kernels_past_the_grid_cap():
    """ts_act_pieces and ts_split_pieces launch at most 16384 workgroups of 256 threads and stride over the rest.  8192 rows of
    n = 4096 are 8,388,608 four-element items: twice the cap, the smallest size at which every thread takes a second item.  The
    pieces of the whole equal the pieces of its two halves computed by launches below the cap, and split_ref / the bound on the
    rows around the seam and at both ends."""
    lib = _ffi.load()
    rows, n = ec.GRID_STRIDE_ROWS, ec.GRID_STRIDE_N
    assert rows * (n // 4) == 2 * ec.GRID_CAP_THREADS
    g = torch.Generator(device="cpu").manual_seed(21)
    x = (torch.randn((rows, n), generator=g) * 2.0).cuda()
    bias = torch.randn(n, generator=g).cuda()
    half = rows // 2
    sample = torch.tensor([0, 1, half - 1, half, half + 1, rows - 2, rows - 1], device="cuda")
    # ts_split_pieces
    whole, parts = ec.guarded((rows, 3 * n), BF16, align=8), ec.guarded((rows, 3 * n), BF16, align=8)
    _ffi.check(lib.ts_split_pieces(0, P(x), rows, n, 0, P(whole), stream()))
    for r0 in (0, half):
        _ffi.check(lib.ts_split_pieces(0, P(x[r0:]), half, n, 0, P(parts[r0:]), stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(whole).any() and ec.same_bits(whole, parts)
    assert ec.same_bits(whole[sample], ec.split_ref(x[sample]))
    ec.assert_margins(whole, parts)
    # ts_act_pieces (kind 0: one input row per output row)
    whole.fill_(float("nan"))
    parts.fill_(float("nan"))
    _ffi.check(lib.ts_act_pieces(0, P(x), P(bias), rows, n, 0, P(whole), stream()))
    for r0 in (0, half):
        _ffi.check(lib.ts_act_pieces(0, P(x[r0:]), P(bias), half, n, 0, P(parts[r0:]), stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(whole).any() and ec.same_bits(whole, parts)
    ec.check_act_pieces(whole[sample], x[sample], bias, 0)
    ec.assert_margins(whole, parts)
