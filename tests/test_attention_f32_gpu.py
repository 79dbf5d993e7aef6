"""ts_attention_float (attention_f32_kernel, theoremsearch_amd/csrc/kernels_attention_f32.h) and ts_attention_tiled
(attention_f32_tiled_kernel, kernels_attention_tiled.h), six instantiations each, against tests/attention_f32_common.py
(tests/test_attention_f32_model_cpu.py shows what each check rejects).  B = 3, heads (4, 2, 64 / 128 / 256) plus one wide key / value
group (8, 1, 128), every length next to a 16-token tile edge, a 64-query block edge and a chunk edge, three or more chunks,
ts_attention_float's limit and one past it, 1 / 2 / 3 / 4 waves of attention_f32_kernel, causal and not, under the eight mask kinds of
attention_bf16_tiled_common.long_masks.  Direct calls; the context and its bf16 pieces are both requested into sentinel-filled
buffers whose margins must come back untouched after every launch:
1. the case list reaches all twelve instantiations;
2. selectors - fp32 inputs whose softmax is exactly one-hot in the kernels' tile-wise arithmetic, every excluded key 0x7F7F0000 in K
   and V: the context is the picked V row bit for bit, the pieces are split_ref of it, rows without an allowed key are zeros,
   nothing is NaN / Inf although the excluded keys' scores overflow;
3. the same with a projection bias that is zero on Q and K and random on V: fp32(V[pick] + bias_v) bit for bit;
4. random inputs (with a projection bias over Q, K and V; excluded keys 0x7F7F0000) and the ones column: every element within
   af.LIMIT[hd] units of 2^-24 (A + |want|) of the fp64 reference, also at 1,025 and 2,049 tokens;
5. right padding to the next chunk with masked 0x7F7F0000 tokens, and a key / value group launched alone, change no bit;
6. what LDS held before (+Inf in every V^T image on every compute unit) changes no bit of a selector with a ragged last tile;
7. a call that asks for the pieces alone writes the same pieces."""
import ctypes as C

import pytest
import torch

import attention_f32_common as af
import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
B = af.B
ENTRY = {"float": "ts_attention_float", "tiled": "ts_attention_tiled"}
config = pytest.mark.parametrize("entry,hq,hkv,hd", [(e,) + s for e in af.ENTRIES for s in af.HEADS], ids=lambda v: str(v))
config_wide = pytest.mark.parametrize("entry,hq,hkv,hd", [(e,) + s for e in af.ENTRIES for s in af.HEADS + (af.WIDE_GROUP,)], ids=lambda v: str(v))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(t):
    return None if t is None else t.cuda()


def launch(entry, qkv, bias, mask, batch, S, hq, hkv, hd, causal, out, pieces):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(getattr(_ffi.load(), ENTRY[entry])(0, P(qkv), P(bias), P(mask), batch, S, hq, hkv, hd, 1 if causal else 0, hd ** -0.5, P(out),
                                                  P(pieces), st))


def split(y):
    """encoder_common.split_ref's [hi | lo | hi] with torch's rounding, on the device y lives on."""
    hi = y.bfloat16()
    return torch.cat((hi, (y - hi.float()).bfloat16(), hi), dim=-1)


def attend(entry, qkv, mask, hq, hkv, hd, causal, bias=None):
    """(context, pieces) of the entry for device tensors, from guarded buffers whose margins are checked."""
    batch, S, width = qkv.shape
    assert width == (hq + 2 * hkv) * hd and qkv.dtype == F32 and qkv.is_contiguous() and (mask is None or mask.is_contiguous())
    assert entry == "tiled" or S <= af.FLOAT_MAX_SEQ[hd]
    out = ec.guarded((batch, S, hq * hd), F32)
    pieces = ec.guarded((batch * S, 3 * hq * hd), BF16, align=8)
    launch(entry, qkv, bias, mask, batch, S, hq, hkv, hd, causal, out, pieces)
    torch.cuda.synchronize()
    ec.assert_margins(out, pieces)
    return out, pieces


def test_the_case_list_reaches_all_twelve_instantiations():
    assert af.reached_instantiations() == af.all_instantiations() and len(af.all_instantiations()) == 12
    for hd in af.CHUNK:
        assert {af.float_waves(S) for S in af.lengths("float", hd)} == {1, 2, 3, 4}
        assert max(af.lengths("float", hd)) == af.FLOAT_MAX_SEQ[hd] and af.FLOAT_MAX_SEQ[hd] + 1 in af.lengths("tiled", hd)


def selector_sweep(entry, hq, hkv, hd, lengths, picks, vbias):
    cases = keyless = 0
    for S in lengths:
        for kind in af.MASK_KINDS:
            for causal in (False, True):
                for pick in picks:
                    tag = (entry, hq, hkv, hd, S, kind, causal, pick, vbias)
                    qkv, bias, mask, has_key, want = af.selector_case(hq, hkv, hd, S, kind, causal, pick, vbias)
                    want, has_key = want.cuda(), has_key.cuda()
                    got, pieces = attend(entry, qkv.cuda(), dev(mask), hq, hkv, hd, causal, dev(bias))
                    assert torch.isfinite(got).all(), (tag, "NaN / Inf: an excluded key leaked, or a maximum was taken over excluded scores")
                    if not ec.same_bits(got, want):
                        rows = (ec.bits(got) != ec.bits(want)).view(B, S, hq, hd).any(-1).nonzero()
                        raise AssertionError((tag, f"{len(rows)} (sequence, query, head) rows are not the picked V row, first {rows[0].tolist()}",
                                              "has a key", bool(has_key[rows[0][0], rows[0][1]])))
                    assert not got[~has_key].any(), tag                              # (zeros in `want`: compared above, bit for bit)
                    assert ec.same_bits(pieces, split(want.view(B * S, -1))), (tag, "pieces are not split_ref(context)")
                    if S == 17 and pick == picks[0]:
                        assert ec.same_bits(pieces.cpu(), ec.split_ref(got.view(B * S, -1)))
                    if kind == "keyless":
                        assert not has_key[B - 1].any()
                    keyless += int((~has_key).sum())
                    cases += 1
    return cases, keyless


@config
def test_selectors_come_back_bit_for_bit(entry, hq, hkv, hd, capsys):
    cases, keyless = selector_sweep(entry, hq, hkv, hd, af.lengths(entry, hd), af.PICKS, False)
    assert keyless > 0
    with capsys.disabled():
        print(f"\n{ENTRY[entry]} {hq}/{hkv} x {hd}: {cases} selector cases exact, {keyless} keyless rows exactly zero", end="")


@config
def test_v_bias_selectors_come_back_bit_for_bit(entry, hq, hkv, hd, capsys):
    """V's share of the projection bias at every length of the list - every chunk edge of the tiled kernel's staging: the picked row
    plus bias_v, rounded once."""
    cases, keyless = selector_sweep(entry, hq, hkv, hd, af.lengths(entry, hd), af.PICKS, True)
    assert keyless > 0
    with capsys.disabled():
        print(f"\n{ENTRY[entry]} {hq}/{hkv} x {hd}: {cases} V-bias selector cases exact, {keyless} keyless rows exactly zero", end="")


@pytest.mark.parametrize("entry", af.ENTRIES)
def test_selectors_of_a_wide_group_come_back_bit_for_bit(entry, capsys):
    """Eight query heads over one key / value head: the workgroups of the group are neighbours in the grid and read the same K and V."""
    hq, hkv, hd = af.WIDE_GROUP
    Cn = af.CHUNK[hd]
    cases, keyless = selector_sweep(entry, hq, hkv, hd, (17, Cn + 1, 3 * Cn + 17), af.PICKS, False)
    more, keyless2 = selector_sweep(entry, hq, hkv, hd, (17, Cn + 1, 3 * Cn + 17), ("random",), True)
    assert keyless > 0 and keyless2 > 0
    with capsys.disabled():
        print(f"\n{ENTRY[entry]} {hq}/{hkv} x {hd}: {cases} selector and {more} V-bias selector cases exact", end="")


@config
def test_random_inputs_and_the_ones_column_within_the_limit(entry, hq, hkv, hd, capsys):
    worst = {"random": 0.0, "ones": 0.0, "random long": 0.0, "ones long": 0.0}
    bad, keyless, held = [], 0, None
    for Bn, S, kind in af.bound_cases(entry, hq, hkv, hd):
        if held is None or held[0] != (Bn, S):
            qkv, bias, masks = af.random_inputs(Bn, S, hq, hkv, hd)
            held = ((Bn, S), qkv.cuda(), bias.cuda(), masks)
        _, qkv, bias, masks = held
        mask = dev(masks[kind])
        for ones in (False, True):
            x = af.masked(qkv, mask, hq, hkv, hd, ones=ones)
            for causal in (False, True):
                tag = (entry, hq, hkv, hd, Bn, S, kind, causal, "ones" if ones else "random")
                want, has_key, u = af.unit(x, mask, hq, hkv, hd, causal, bias=None if ones else bias, ones=ones)
                got, pieces = attend(entry, x, mask, hq, hkv, hd, causal, None if ones else bias)
                assert torch.isfinite(got).all(), tag
                assert not got[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
                assert ec.same_bits(pieces, split(got.view(Bn * S, -1))), (tag, "pieces are not split_ref(context)")
                keyless += int((~has_key).sum())
                r = af.worst_r(got, want, has_key, u)
                key = ("ones" if ones else "random") + (" long" if S > 513 else "")
                worst[key] = max(worst[key], r)
                if r > af.LIMIT[hd]:
                    bad.append((tag, round(r, 2)))
    with capsys.disabled():
        print(f"\n{ENTRY[entry]} {hq}/{hkv} x {hd}: worst r " + ", ".join(f"{v:.2f} ({k})" for k, v in worst.items() if v or "long" not in k)
              + f" of LIMIT {af.LIMIT[hd]:g}; {keyless} keyless rows exactly zero", end="")
    assert not bad, bad
    assert keyless > 0


@config
def test_right_padding_to_the_next_chunk_changes_no_bit(entry, hq, hkv, hd):
    """A batch at S0 tokens re-laid at the next multiple of the chunk (ts_attention_float: up to its limit) with masked 0x7F7F0000
    tokens behind it: the first S0 rows are the same bits.  The extra keys' scores overflow and are discarded by a select, each adds
    an exact 0 to the row's sum and 0 x finite to the accumulators; a whole extra tile rescales by exactly 1."""
    Cn = af.CHUNK[hd]
    for S0 in (17, Cn - 1, Cn, 2 * Cn + 1):
        qkv0, bias, masks = af.random_inputs(B, S0, hq, hkv, hd)
        qkv0, bias = qkv0.cuda(), bias.cuda()
        S = (S0 // Cn + 1) * Cn
        if entry == "float":
            S = min(S, af.FLOAT_MAX_SEQ[hd])
        assert S > S0
        for kind in ("none", "holes"):
            mask0 = dev(masks[kind])
            x0 = af.masked(qkv0, mask0, hq, hkv, hd)
            x, mask = af.pad_right(x0, S)
            if mask0 is not None:
                mask[:, :S0] = mask0
            for causal in (False, True):
                tag = (entry, hq, hkv, hd, S0, S, kind, causal)
                base, base_pieces = attend(entry, x0, mask0, hq, hkv, hd, causal, bias)
                got, pieces = attend(entry, x, mask, hq, hkv, hd, causal, bias)
                assert torch.isfinite(base).all() and torch.isfinite(got[:, :S0]).all(), tag
                assert ec.same_bits(got[:, :S0], base), (tag, (got[:, :S0] - base).abs().max().item())
                assert ec.same_bits(pieces.view(B, S, -1)[:, :S0], base_pieces.view(B, S0, -1)), tag


@config_wide
def test_a_group_alone_equals_the_group_in_the_batch(entry, hq, hkv, hd):
    """Each (sequence, key / value group) as a call of its own (B = 1, hq = per_kv, hkv = 1) gives the bits it gave inside the batch."""
    per_kv = hq // hkv
    Cn = af.CHUNK[hd]
    for S in (65, 2 * Cn + 1):
        qkv, bias, masks = af.random_inputs(B, S, hq, hkv, hd)
        qkv, bias = qkv.cuda(), bias.cuda()
        for kind in ("none", "left"):
            mask = dev(masks[kind])
            x = af.masked(qkv, mask, hq, hkv, hd)
            for causal in (False, True):
                batch = attend(entry, x, mask, hq, hkv, hd, causal, bias)[0].view(B, S, hkv, per_kv * hd)
                assert torch.isfinite(batch).all()
                for b in range(B):
                    for kvh in range(hkv):
                        one, _ = attend(entry, af.alone(x, b, hq, hkv, hd, kvh), None if mask is None else mask[b:b + 1].contiguous(), per_kv, 1, hd,
                                        causal, af.alone(bias.view(1, 1, -1), 0, hq, hkv, hd, kvh).reshape(-1))
                        assert ec.same_bits(one[0], batch[b, :, kvh]), (entry, hq, hkv, hd, S, kind, causal, b, kvh)


@config
def test_what_lds_held_before_changes_no_number(entry, hq, hkv, hd):
    """A selector with a ragged last tile directly after a call that leaves +Inf in every V^T image on every compute unit (Q = K = 0,
    V = +Inf, ts_attention_float at 128 tokens, ts_attention_tiled at two full chunks; at least four workgroups per compute unit): a
    stale V^T column past S against a zero weight would give NaN.  A correct kernel reads nothing it did not write."""
    Cn = af.CHUNK[hd]
    Sp = 128 if entry == "float" else 2 * Cn
    groups = hq * (1 if entry == "float" else -(-Sp // 64))
    nb = -(-4 * torch.cuda.get_device_properties(0).multi_processor_count // groups)
    inf = torch.zeros((nb, Sp, (hq + 2 * hkv) * hd), dtype=F32, device="cuda")
    inf.view(nb, Sp, hq + 2 * hkv, hd)[:, :, hq + hkv:] = float("inf")
    sink = ec.guarded((nb, Sp, hq * hd), F32)
    for S in ((17, 113) if entry == "float" else (17, Cn + 1, 2 * Cn + 17)):
        for kind in ("none", "left"):
            for causal in (False, True):
                qkv, _, mask, has_key, want = af.selector_case(hq, hkv, hd, S, kind, causal, "random")
                qkv, mask, want = qkv.cuda(), dev(mask), want.cuda()
                launch(entry, inf, None, None, nb, Sp, hq, hkv, hd, causal, sink, None)
                got, pieces = attend(entry, qkv, mask, hq, hkv, hd, causal)
                ec.assert_margins(sink)
                assert torch.isfinite(got).all() and ec.same_bits(got, want), (entry, hq, hkv, hd, S, kind, causal)
                assert ec.same_bits(pieces, split(want.view(B * S, -1)))
    assert not torch.isfinite(sink).any()                                            # (the poisoning call ran: Inf, or NaN on a causal diagonal tile)


@config_wide
def test_a_call_for_the_pieces_alone_writes_the_same_pieces(entry, hq, hkv, hd):
    Cn = af.CHUNK[hd]
    S = 2 * Cn + 1
    qkv, bias, masks = af.random_inputs(B, S, hq, hkv, hd)
    qkv, bias, mask = qkv.cuda(), bias.cuda(), masks["holes"].cuda()
    x = af.masked(qkv, mask, hq, hkv, hd)
    for causal in (False, True):
        out, pieces = attend(entry, x, mask, hq, hkv, hd, causal, bias)
        only = ec.guarded((B * S, 3 * hq * hd), BF16, align=8)
        launch(entry, x, bias, mask, B, S, hq, hkv, hd, causal, None, only)
        torch.cuda.synchronize()
        ec.assert_margins(only)
        assert ec.same_bits(only, pieces) and ec.same_bits(pieces, split(out.view(B * S, -1))), (entry, hq, hkv, hd, causal)
