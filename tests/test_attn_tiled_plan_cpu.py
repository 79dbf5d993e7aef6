"""ts_attention_tiled without a GPU:
* its host decisions (theoremsearch_amd/csrc/encoder_plan.h: chunk sizes, LDS, tiles, query blocks, grid, the refusals) are plain
  integer arithmetic in a header that needs no HIP.  tests/attn_tiled_plan_check.cpp checks them in a program of its own, built
  with the host compiler under the address and undefined-behaviour sanitizers and run as a child process; nothing of it is
  loaded into Python.  The program prints the chunk sizes and the token limit, and fused_forward's mirrors are held against them;
* the helper that picks the fp32 attention of a forward ("float" / "tiled" / None) at the edges of each kernel's range;
* the argument contract of ts_attention_tiled: ts_attention_float's checks, all before the device check (the library loads
  without a device; a refusal never dereferences a pointer, so aligned fake ones do)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

import encoder_common as ec
from conftest import ROOT, gpu_available
from theoremsearch_amd import _ffi
from theoremsearch_amd import fused_forward as ff

P = 0x7F0000001000                                            # a 16-byte aligned address no refusal dereferences


def test_tiled_plan_checks_pass_under_the_host_sanitizers_and_the_python_mirrors_match(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "attn_tiled_plan_check"
    # the sanitizers' runtimes linked into the program (clang's default): it starts whatever else the loader brings in
    static_rt = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         *static_rt, "-I", os.path.join(ROOT, "theoremsearch_amd", "csrc"), os.path.join(ROOT, "tests", "attn_tiled_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=280)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
    words = [line.split() for line in run.stdout.splitlines()]
    chunk = {int(w[1]): int(w[2]) for w in words if w and w[0] == "chunk"}
    max_seq = [int(w[1]) for w in words if w and w[0] == "max_seq"]
    assert chunk == ff._TILED_CHUNK and max_seq == [ff._TILED_MAX_SEQ], (chunk, max_seq)
    assert set(ff._TILED_CHUNK) == set(ff._FLOAT_ATTENTION_MAX_SEQ) == set(ff._TILED_ROUTED_MAX_SEQ)


def test_the_helper_names_the_kernel_of_every_range(monkeypatch):
    monkeypatch.delenv("TS_ENCODER_ATTENTION", raising=False)
    f32, bf16 = torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.bfloat16)
    for hd, old in ff._FLOAT_ATTENTION_MAX_SEQ.items():
        assert ff.fp32_attention_kind(f32, 1, hd) == "float" and ff.fp32_attention_kind(f32, old, hd) == "float"
        routed = ff._TILED_ROUTED_MAX_SEQ[hd]                     # where the family keeps torch's attention: a measured loss
        assert old < routed <= ff._TILED_MAX_SEQ
        assert ff.fp32_attention_kind(f32, old + 1, hd) == "tiled" and ff.fp32_attention_kind(f32, routed, hd) == "tiled"
        assert ff.fp32_attention_kind(f32, routed + 1, hd) is None and ff.fp32_attention_kind(f32, ff._TILED_MAX_SEQ + 1, hd) is None
        for S in (1, old, old + 1):
            assert ff.fp32_attention_kind(bf16, S, hd) is None
            assert ff.float_attention_applies(f32, S, hd) == (S <= old)                     # unchanged
    for hd in (32, 96, 512):
        assert ff.fp32_attention_kind(f32, 16, hd) is None and ff.fp32_attention_kind(f32, 1000, hd) is None
    assert ff._TILED_ROUTED_MAX_SEQ == {64: 32768, 128: 32768, 256: 256}
    monkeypatch.setenv("TS_ENCODER_ATTENTION", "0")
    for hd, old in ff._FLOAT_ATTENTION_MAX_SEQ.items():
        assert ff.fp32_attention_kind(f32, old, hd) is None and ff.fp32_attention_kind(f32, old + 1, hd) is None


def _p(v):
    return None if v is None else C.c_void_p(v)


def tiled(lib, qkv=P, qkv_bias=None, mask=None, batch=2, seq=16, hq=4, hkv=2, hd=64, causal=0, scale=0.125, out=P, pieces=None):
    return lib.ts_attention_tiled(0, _p(qkv), _p(qkv_bias), _p(mask), batch, seq, hq, hkv, hd, causal, scale, _p(out), _p(pieces), None)


def floating(lib, qkv=P, qkv_bias=None, mask=None, batch=2, seq=16, hq=4, hkv=2, hd=64, causal=0, scale=0.125, out=P, pieces=None):
    return lib.ts_attention_float(0, _p(qkv), _p(qkv_bias), _p(mask), batch, seq, hq, hkv, hd, causal, scale, _p(out), _p(pieces), None)


def test_tiled_refusals_come_before_the_device_check_and_are_ts_attention_floats():
    lib = _ffi.load()
    inv, uns = ec.TS_ERR_INVALID, ec.TS_ERR_UNSUPPORTED
    refused = (dict(qkv=None), dict(out=None, pieces=None), dict(qkv_bias=P + 8), dict(batch=-1), dict(seq=0), dict(seq=-5), dict(hq=0),
               dict(hkv=0), dict(hq=6, hkv=4), dict(qkv=P + 8), dict(out=P + 8), dict(out=P + 4), dict(pieces=P + 4), dict(out=None, pieces=P + 4),
               dict(scale=0.0), dict(scale=-0.125), dict(scale=float("nan")))
    for kw in refused:
        assert tiled(lib, **kw) == inv, kw
        text = lib.ts_last_error()
        assert floating(lib, **kw) == inv and lib.ts_last_error() == text, kw                 # the same refusal, the same words
    # order: NULL, the bias, the counts, the shape, the alignment, the scale - as ts_attention_float
    for kw, word in ((dict(qkv=None, qkv_bias=P + 8, seq=0), b"NULL"), (dict(qkv_bias=P + 8, seq=0, hd=32), b"qkv_bias"),
                     (dict(seq=0, hd=32, out=P + 8), b"seq = 0"), (dict(hd=32, out=P + 8, scale=0.0), b"head size"),
                     (dict(out=P + 8, scale=0.0), b"16-byte aligned"), (dict(scale=0.0), b"scale")):
        rc = tiled(lib, **kw)
        assert rc in (inv, uns) and word in lib.ts_last_error(), (kw, lib.ts_last_error())
        assert floating(lib, **kw) == rc and word in lib.ts_last_error(), kw
    # what is not served: another head size, one token past the limit, a grid past 31 bits
    for kw in (dict(hd=32), dict(hd=0), dict(hd=96), dict(hd=512), dict(seq=32769), dict(hd=128, seq=32769), dict(hd=256, seq=2 ** 31 - 1),
               dict(batch=2 ** 20, seq=32768, hq=4, hkv=4), dict(batch=2 ** 31 - 1, seq=65, hq=1, hkv=1)):
        assert tiled(lib, **kw) == uns, kw
        assert b"64 / 128 / 256" in lib.ts_last_error() and b"32768 tokens" in lib.ts_last_error(), lib.ts_last_error()
    # nothing to do is not an error and needs no device - but it is checked like any other call
    assert tiled(lib, batch=0) == 0 and tiled(lib, batch=0, hd=256, seq=32768, out=None, pieces=P + 8) == 0
    assert tiled(lib, batch=0, hd=32) == uns and tiled(lib, batch=0, out=P + 8) == inv and tiled(lib, batch=0, scale=0.0) == inv


@pytest.mark.skipif(gpu_available(), reason="fake pointers: only where the device check refuses the call")
def test_valid_tiled_arguments_reach_the_device_check():
    lib = _ffi.load()
    nod = ec.TS_ERR_NODEVICE
    for hd, seq in ((64, 32768), (128, 257), (256, 129), (64, 1), (128, 256), (256, 128)):
        assert tiled(lib, hd=hd, seq=seq) == nod, (hd, seq)
        assert tiled(lib, hd=hd, seq=seq, causal=1, qkv_bias=P, mask=P, pieces=P + 8) == nod, (hd, seq)
        assert tiled(lib, hd=hd, seq=seq, out=None, pieces=P) == nod, (hd, seq)
    assert tiled(lib, batch=2 ** 31 - 1, seq=64, hq=1, hkv=1) == nod                            # 2^31 - 1 blocks
    # at each of the forwards' named limits the call gets this far; one step past it, it is refused
    for hd in ff._TILED_CHUNK:
        assert tiled(lib, hd=hd, seq=ff._TILED_MAX_SEQ) == nod and tiled(lib, hd=hd, seq=ff._TILED_MAX_SEQ + 1) == ec.TS_ERR_UNSUPPORTED
