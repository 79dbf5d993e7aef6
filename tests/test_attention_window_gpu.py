"""ts_attention_flash_window and ts_attention_tiled_window (attention_bf16_tiled_kernel / attention_f32_tiled_kernel with WINDOW, twelve new
instantiations) against tests/attention_window_common.py (tests/test_attention_window_model_cpu.py shows what each check rejects).
Heads of 64 / 128 / 256, causal and not, no mask / right padding / left padding / holes, at the smallest lengths and windows at which
chunks are skipped on both sides at each head size; every output lies in a sentinel-filled buffer whose margins must come back
untouched:
1. equiv - row q of the windowed call is row q of the PARENT entry called with the key mask window_mask_for(q), bit for bit, at up to
   32 probed rows per case (both ends, rows whose window edge falls on a tile, query-block or chunk edge, random ones); fp32 also
   compares the pieces, and runs with a projection bias under one mask kind; once per head shape at 1,025 tokens, W = 257;
2. bound - every row within the parent's bound of the fp64 reference with the window; rows without a key are zeros;
3. window >= seq returns the parent entry's bits;
4. window < 1 is refused, and the parents' refusals come back unchanged with a window given."""
import ctypes as C

import pytest
import torch

import attention_window_common as aw
import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPE = {"flash": BF16, "tiled": F32}
BIAS_KIND = "holes"                                  # the mask kind under which the fp32 entry also gets a projection bias
entries = pytest.mark.parametrize("entry", aw.ENTRIES)
shapes = pytest.mark.parametrize("hq,hkv,hd", aw.HEADS, ids=lambda v: str(v))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(t):
    return None if t is None else t.cuda()


def attend(entry, window, qkv, bias, mask, hq, hkv, hd, causal):
    """(out, pieces or None) of the windowed entry, or of its parent (window=None), for device tensors, in guarded buffers."""
    batch, S, width = qkv.shape
    assert width == (hq + 2 * hkv) * hd and qkv.dtype == DTYPE[entry] and qkv.is_contiguous() and (mask is None or mask.is_contiguous())
    lib, st = _ffi.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = ec.guarded((batch, S, hq * hd), DTYPE[entry])
    win = () if window is None else (int(window),)
    pieces = None
    if entry == "flash":
        fn = lib.ts_attention_flash if window is None else lib.ts_attention_flash_window
        _ffi.check(fn(0, P(qkv), P(mask), batch, S, hq, hkv, hd, 1 if causal else 0, *win, hd ** -0.5, P(out), st))
    else:
        pieces = ec.guarded((batch * S, 3 * hq * hd), BF16)
        fn = lib.ts_attention_tiled if window is None else lib.ts_attention_tiled_window
        _ffi.check(fn(0, P(qkv), P(bias), P(mask), batch, S, hq, hkv, hd, 1 if causal else 0, *win, hd ** -0.5, P(out), P(pieces), st))
    torch.cuda.synchronize()
    ec.assert_margins(out, *(() if pieces is None else (pieces,)))
    return out, pieces


def check_equiv(entry, qkv, bias, mask, S, W, hq, hkv, hd, causal, rows, tag):
    """qkv, bias, mask on the CPU.  Row (b, q) of the windowed call against row q of the parent under window_mask_for(q)."""
    got, got_p = attend(entry, W, qkv.cuda(), dev(bias), dev(mask), hq, hkv, hd, causal)
    rep, masks, index = aw.parent_batch(qkv, mask, S, W, rows)
    assert len(index) <= 32
    want, want_p = attend(entry, None, rep.cuda(), dev(bias), masks.cuda(), hq, hkv, hd, causal)
    a, b = aw.probed(got, index, False), aw.probed(want, index, True)
    assert torch.isfinite(a.float()).all(), tag
    if not ec.same_bits(a, b):
        bad = [index[i] for i in (ec.bits(a) != ec.bits(b)).any(-1).nonzero().flatten().tolist()]
        raise AssertionError(f"{tag}: rows (sequence, query) {bad[:8]} differ from the parent under the equivalent key mask")
    if got_p is not None:
        n = len(index)
        ap = aw.probed(got_p.view(qkv.shape[0], S, -1), index, False)
        bp = aw.probed(want_p.view(n, S, -1), index, True)
        assert ec.same_bits(ap, bp), (tag, "pieces")


@entries
@shapes
def test_rows_equal_the_parent_under_the_equivalent_key_mask_bit_for_bit(entry, hq, hkv, hd):
    cases = 0
    for S in aw.lengths(hd):
        qkv, bias, masks = aw.inputs(entry, aw.B, S, hq, hkv, hd)
        for W in aw.windows(hd, S):
            rows = aw.probe_rows(S, W, hd)
            for kind in aw.MASK_KINDS:
                for causal in (False, True):
                    use_bias = bias if kind == BIAS_KIND else None
                    check_equiv(entry, qkv, use_bias, masks[kind], S, W, hq, hkv, hd, causal, rows, (entry, hq, hkv, hd, S, W, kind, causal))
                    cases += 1
    assert cases == len(list(aw.equiv_cases(hd)))


@entries
@shapes
def test_a_long_sequence_equals_the_parent_bit_for_bit(entry, hq, hkv, hd):
    S, W = aw.LONG
    qkv, bias, masks = aw.inputs(entry, 1, S, hq, hkv, hd)
    rows = aw.probe_rows(S, W, hd, 32)
    for causal in (False, True):
        check_equiv(entry, qkv, None, masks["holes"], S, W, hq, hkv, hd, causal, rows, (entry, hq, hkv, hd, S, W, causal))


@entries
@shapes
def test_every_row_within_the_parents_bound_of_the_fp64_reference(entry, hq, hkv, hd, capsys):
    worst = 0.0
    for S, W, kind, causal in aw.bound_cases(hd):
        qkv, bias, masks = aw.inputs(entry, aw.B, S, hq, hkv, hd)
        mask = masks[kind]
        got, _ = attend(entry, W, qkv.cuda(), dev(bias), dev(mask), hq, hkv, hd, causal)
        r = aw.bound_ratio(entry, got.cpu(), qkv, aw.allowed_w(mask, aw.B, S, causal, W), hq, hkv, hd, bias)
        worst = max(worst, r)
        with capsys.disabled():
            print(f"\n  window bound {entry} {(hq, hkv, hd)} S={S} W={W} {kind} causal={causal}: ratio {r:.3f} of limit {aw.limit(entry, hd)}", end="")
        assert r <= aw.limit(entry, hd), (entry, hq, hkv, hd, S, W, kind, causal, r)
    assert worst > 0.0


@entries
@shapes
def test_a_window_that_reaches_the_sequence_returns_the_parents_bits(entry, hq, hkv, hd):
    S = 2 * aw.CHUNK[hd] + 1
    qkv, bias, masks = aw.inputs(entry, aw.B, S, hq, hkv, hd)
    for causal in (False, True):
        want, want_p = attend(entry, None, qkv.cuda(), dev(bias), dev(masks["holes"]), hq, hkv, hd, causal)
        for W in (S, S + 1, 2 ** 31 - 1):
            got, got_p = attend(entry, W, qkv.cuda(), dev(bias), dev(masks["holes"]), hq, hkv, hd, causal)
            assert ec.same_bits(got, want), (entry, hd, causal, W)
            assert got_p is None or ec.same_bits(got_p, want_p), (entry, hd, causal, W, "pieces")


def test_window_below_one_is_refused_and_the_parents_refusals_come_back_unchanged():
    lib = _ffi.load()
    x = torch.zeros((2, 16, 8 * 64), dtype=BF16, device="cuda")
    xf = torch.zeros((2, 16, 8 * 64), dtype=F32, device="cuda")

    def flash(window, qkv=x, batch=2, seq=16, hq=4, hkv=2, hd=64, scale=0.125, off=0):
        args = (0, P(qkv), None, batch, seq, hq, hkv, hd, 0)
        tail = (scale, C.c_void_p(x.data_ptr() + off), None)
        return lib.ts_attention_flash(*args, *tail) if window is None else lib.ts_attention_flash_window(*args, window, *tail)

    def tiled(window, qkv=xf, batch=2, seq=16, hq=4, hkv=2, hd=64, scale=0.125, off=0):
        args = (0, P(qkv), None, None, batch, seq, hq, hkv, hd, 0)
        tail = (scale, C.c_void_p(xf.data_ptr() + off), None, None)
        return lib.ts_attention_tiled(*args, *tail) if window is None else lib.ts_attention_tiled_window(*args, window, *tail)

    for fn in (flash, tiled):
        assert fn(0) == ec.TS_ERR_INVALID and b"window" in lib.ts_last_error()
        assert fn(-1) == ec.TS_ERR_INVALID and fn(-2 ** 31) == ec.TS_ERR_INVALID
        for kw, code in ((dict(hd=96), ec.TS_ERR_UNSUPPORTED), (dict(seq=0), ec.TS_ERR_INVALID), (dict(seq=32769), ec.TS_ERR_UNSUPPORTED),
                         (dict(batch=2 ** 31 - 1, seq=65, hq=1, hkv=1), ec.TS_ERR_UNSUPPORTED), (dict(off=8), ec.TS_ERR_INVALID),
                         (dict(scale=0.0), ec.TS_ERR_INVALID), (dict(hq=6, hkv=4), ec.TS_ERR_INVALID), (dict(qkv=None), ec.TS_ERR_INVALID)):
            parent = fn(None, **kw)
            text = lib.ts_last_error()
            for W in (5, 257):
                assert fn(W, **kw) == parent == code and lib.ts_last_error() == text, (fn.__name__, kw, W)
        assert fn(5, batch=0) == 0
