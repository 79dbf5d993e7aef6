"""ts_qk_norm_rope, ts_gemma_qk_norm_rope, ts_swiglu and ts_geglu called directly, in bf16 and fp32, against fp64 references
with a bound on EVERY element (tests/encoder_common.py; the references, the bounds and their teeth are checked without a GPU
in tests/test_encoder_ref_cpu.py):
* rotary: item counts that leave idle head groups and idle waves in the last workgroup, seq > tokens, tokens no multiple of
  seq, seq == 1, the models' own head counts; tables of independent angles (the two halves of a row differ, no sin is small),
  an all-zero head, a head where eps dominates the mean square, a large one; value heads bit for bit; a call over the first t
  tokens against the same tokens of a larger call, bit for bit (idle groups against full waves);
* gated activations: the smallest width (one 16-byte access), odd access counts, 1 / 5 / 259 rows, special gate and up values,
  and past the grid cap, where every thread strides.
Every buffer lies in a sentinel-filled allocation whose margins must come back untouched."""
import ctypes as C

import pytest
import torch

import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 1}
NAME = {F32: "fp32", BF16: "bf16"}
ROPE_ENTRY = {False: "ts_qk_norm_rope", True: "ts_gemma_qk_norm_rope"}
GATED_ENTRY = {1: "ts_swiglu", 2: "ts_geglu"}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(t):
    """A guarded device copy of a CPU tensor."""
    d = ec.guarded(tuple(t.shape), t.dtype)
    d.copy_(t)
    return d


def rope(gemma, qkv, wq, wk, cos, sin, tokens, seq, hq, hkv):
    """The entry point, in place on the first `tokens` rows of `qkv`."""
    fn = getattr(_ffi.load(), ROPE_ENTRY[gemma])
    _ffi.check(fn(0, P(qkv), P(wq), P(wk), P(cos), P(sin), ec.ROPE_EPS, tokens, seq, hq, hkv, ec.ROPE_HEAD[gemma], CODE[qkv.dtype], stream()))


def gated(kind, gate_up, rows, inter, out):
    fn = getattr(_ffi.load(), GATED_ENTRY[kind])
    _ffi.check(fn(0, P(gate_up), rows, inter, CODE[gate_up.dtype], P(out), stream()))


@pytest.mark.parametrize("dtype", (BF16, F32), ids=lambda d: NAME[d])
@pytest.mark.parametrize("gemma", (False, True), ids=("qwen3", "gemma3"))
def test_qk_norm_rope_against_fp64_on_every_element(gemma, dtype, capsys):
    hd = ec.ROPE_HEAD[gemma]
    worst = 0.0
    for tokens, seq, hq, hkv in ec.ROPE_SHAPES:
        tag = (ROPE_ENTRY[gemma], NAME[dtype], tokens, seq, hq, hkv)
        ins = ec.rope_inputs(tokens, seq, hq, hkv, gemma, dtype)
        qkv, wq, wk, cos, sin = (on_device(t) for t in ins)              # qkv: a clone the call rewrites; `ins` supplies the reference
        rope(gemma, qkv, wq, wk, cos, sin, tokens, seq, hq, hkv)
        torch.cuda.synchronize()
        ec.assert_margins(qkv, wq, wk, cos, sin)
        for d, h in zip((wq, wk, cos, sin), ins[1:]):
            assert ec.same_bits(d, h), (tag, "an operand changed")
        try:
            worst = max(worst, ec.check_rope(qkv.cpu(), *ins, seq, hq, hkv, hd, ec.ROPE_EPS, gemma))
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
    with capsys.disabled():
        print(f"\n{ROPE_ENTRY[gemma]} {NAME[dtype]}: worst error / bound = {worst:.3f} (K = {ec.ROPE_K[(gemma, dtype)]})", end="")


@pytest.mark.parametrize("dtype", (BF16, F32), ids=lambda d: NAME[d])
@pytest.mark.parametrize("gemma", (False, True), ids=("qwen3", "gemma3"))
def test_qk_norm_rope_of_a_prefix_equals_the_prefix_of_a_larger_call(gemma, dtype):
    """The first t tokens do not depend on how many follow: a call with tokens = t (its last wave or workgroup partly idle) returns
    the bits the larger call returns for them, and leaves the rows behind them alone."""
    tokens, seq, hq, hkv = ec.ROPE_PREFIX_SHAPE
    ins = ec.rope_inputs(tokens, seq, hq, hkv, gemma, dtype)
    whole, wq, wk, cos, sin = (on_device(t) for t in ins)
    rope(gemma, whole, wq, wk, cos, sin, tokens, seq, hq, hkv)
    torch.cuda.synchronize()
    ec.check_rope(whole.cpu(), *ins, seq, hq, hkv, ec.ROPE_HEAD[gemma], ec.ROPE_EPS, gemma)
    for t in ec.ROPE_PREFIXES:
        part = on_device(ins[0])
        rope(gemma, part, wq, wk, cos, sin, t, seq, hq, hkv)
        torch.cuda.synchronize()
        ec.assert_margins(part)
        assert ec.same_bits(part[:t], whole[:t]), (ROPE_ENTRY[gemma], NAME[dtype], t, "the prefix differs from the larger call's")
        assert ec.same_bits(part[t:].cpu(), ins[0][t:]), (ROPE_ENTRY[gemma], NAME[dtype], t, "rows past `tokens` were written")
    ec.assert_margins(whole, wq, wk, cos, sin)


@pytest.mark.parametrize("dtype", (BF16, F32), ids=lambda d: NAME[d])
@pytest.mark.parametrize("kind", (1, 2), ids=("swiglu", "geglu"))
def test_gated_activation_against_fp64_on_every_element(kind, dtype, capsys):
    worst = 0.0
    for inter in ec.GATED_WIDTHS[dtype]:
        for rows in ec.GATED_ROWS:
            x = ec.gated_inputs(kind, inter, rows, dtype)
            gate_up, out = on_device(x), ec.guarded((rows, inter), dtype)
            gated(kind, gate_up, rows, inter, out)
            torch.cuda.synchronize()
            ec.assert_margins(gate_up, out)
            assert ec.same_bits(gate_up, x), (GATED_ENTRY[kind], NAME[dtype], inter, rows, "the input changed")
            try:
                worst = max(worst, ec.check_gated(out, x, kind))
            except AssertionError as e:
                raise AssertionError(f"{GATED_ENTRY[kind]} {NAME[dtype]}, inter {inter}, rows {rows}: {e}") from None
    with capsys.disabled():
        print(f"\n{GATED_ENTRY[kind]} {NAME[dtype]}: worst error / bound = {worst:.3f}", end="")


@pytest.mark.parametrize("dtype", (BF16, F32), ids=lambda d: NAME[d])
@pytest.mark.parametrize("kind", (1, 2), ids=("swiglu", "geglu"))
def test_gated_activation_past_the_grid_cap(kind, dtype):
    """ts_swiglu / ts_geglu launch at most 16384 workgroups of 256 threads and stride over the rest.  8192 rows of inter = 4096
    (fp32) / 8192 (bf16) are 8,388,608 16-byte items: twice the cap, the smallest size at which every thread takes a second
    item.  The whole equals its two halves computed by launches below the cap, bit for bit, and the fp64 bound holds on the rows
    at both ends and around the seam."""
    rows, inter = ec.GATED_STRIDE[dtype]
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    assert rows * (inter // vec) == 2 * ec.GRID_CAP_THREADS
    g = torch.Generator(device="cuda").manual_seed(22 + kind)
    gate_up = ec.guarded((rows, 2 * inter), dtype)
    gate_up.copy_(torch.randn((rows, 2 * inter), generator=g, device="cuda", dtype=dtype) * 2.0)
    half = rows // 2
    whole, parts = ec.guarded((rows, inter), dtype), ec.guarded((rows, inter), dtype)
    gated(kind, gate_up, rows, inter, whole)
    for r0 in (0, half):
        gated(kind, gate_up[r0:], half, inter, parts[r0:])
    torch.cuda.synchronize()
    assert not torch.isnan(whole).any() and ec.same_bits(whole, parts)
    sample = torch.tensor([0, 1, half - 1, half, half + 1, rows - 2, rows - 1], device="cuda")
    ec.check_gated(whole[sample], gate_up[sample], kind)
    ec.assert_margins(gate_up, whole, parts)
