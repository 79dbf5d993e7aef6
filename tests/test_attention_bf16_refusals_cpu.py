"""The argument contract of ts_attention_flash (the bf16 attention at any length, encoder_ops.hip) without a GPU: every refusal
comes before the device check (the library loads without a device; a refusal never dereferences a pointer, so aligned fake
ones do), in ts_attention_tiled's order and with its texts where they apply, and the limits fused_forward mirrors are the ones
the library refuses at."""
import ctypes as C

import encoder_common as ec
from theoremsearch_amd import _ffi
from theoremsearch_amd import fused_forward as ff

P = 0x7F0000001000                                            # a 16-byte aligned address no refusal dereferences


def _p(v):
    return None if v is None else C.c_void_p(v)


def flash(lib, qkv=P, mask=None, batch=2, seq=16, hq=4, hkv=2, hd=64, causal=0, scale=0.125, out=P):
    return lib.ts_attention_flash(0, _p(qkv), _p(mask), batch, seq, hq, hkv, hd, causal, scale, _p(out), None)


def test_refusals_come_before_the_device_check():
    lib = _ffi.load()
    inv, uns = ec.TS_ERR_INVALID, ec.TS_ERR_UNSUPPORTED
    for kw in (dict(qkv=None), dict(out=None), dict(batch=-1), dict(seq=0), dict(seq=-5), dict(hq=0), dict(hkv=0), dict(hq=6, hkv=4),
               dict(qkv=P + 8), dict(out=P + 8), dict(out=P + 2), dict(scale=0.0), dict(scale=-0.125), dict(scale=float("nan")),
               dict(hd=96, seq=0), dict(hd=96, qkv=None), dict(hd=96, hq=3, hkv=2)):
        assert flash(lib, **kw) == inv, kw
    # order: NULL, the counts, the shape, the alignment, the scale - as ts_attention_tiled
    for kw, word in ((dict(qkv=None, seq=0), b"NULL"), (dict(seq=0, hd=32, out=P + 8), b"seq = 0"), (dict(hd=32, out=P + 8, scale=0.0), b"head size"),
                     (dict(out=P + 8, scale=0.0), b"16-byte aligned"), (dict(scale=0.0), b"scale")):
        rc = flash(lib, **kw)
        assert rc in (inv, uns) and word in lib.ts_last_error(), (kw, lib.ts_last_error())
    # what is not served: another head size, one token past the limit, a grid past 31 bits; the text names the limits
    for kw in (dict(hd=96), dict(hd=32), dict(hd=0), dict(hd=512), dict(seq=32769), dict(hd=128, seq=32769), dict(hd=256, seq=2 ** 31 - 1),
               dict(batch=2 ** 20, seq=32768, hq=4, hkv=4), dict(batch=2 ** 31 - 1, seq=65, hq=1, hkv=1)):
        assert flash(lib, **kw) == uns, kw
        assert b"64 / 128 / 256" in lib.ts_last_error() and b"32768 tokens" in lib.ts_last_error(), lib.ts_last_error()
    # nothing to do is not an error and needs no device - but it is checked like any other call
    assert flash(lib, batch=0) == 0 and flash(lib, batch=0, hd=256, seq=32768, causal=1, mask=P) == 0
    assert flash(lib, batch=0, hd=96) == uns and flash(lib, batch=0, out=P + 8) == inv and flash(lib, batch=0, scale=0.0) == inv


def test_the_limits_fused_forward_mirrors_are_the_librarys():
    lib = _ffi.load()
    assert set(ff._BF16_TILED_CHUNK) == {64, 128, 256}
    for hd in ff._BF16_TILED_CHUNK:
        # at the limit the call passes every refusal (what comes back is the device check's answer or success, never a refusal
        # of the arguments); one token past it, it is refused
        assert flash(lib, batch=0, hd=hd, seq=ff._BF16_TILED_MAX_SEQ) == 0
        assert flash(lib, batch=0, hd=hd, seq=ff._BF16_TILED_MAX_SEQ + 1) == ec.TS_ERR_UNSUPPORTED
        assert ff._BF16_TILED_ROUTED_MAX_SEQ[hd] <= ff._BF16_TILED_MAX_SEQ
    for hd in (32, 96, 512):
        assert flash(lib, batch=0, hd=hd) == ec.TS_ERR_UNSUPPORTED and ff._BF16_TILED_ROUTED_MAX_SEQ.get(hd, 0) == 0
