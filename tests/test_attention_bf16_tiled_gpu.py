"""ts_attention_flash (attention_bf16_tiled_kernel, theoremsearch_amd/csrc/kernels_attention_bf16_tiled.h: six instantiations) against
tests/attention_bf16_tiled_common.py (tests/test_attention_bf16_tiled_model_cpu.py shows what each check rejects).  B = 3, heads of
64 / 128 / 256 plus one wide key / value group, every length next to a 16-token tile edge, a 64-query block edge and a chunk edge
and three or more chunks, causal and not, under the six mask kinds of encoder_common and two more (a whole chunk of left padding;
right padding that leaves key 0); every output lies in a sentinel-filled buffer whose margins must come back untouched:
1. selectors - inputs whose softmax is exactly one-hot in the kernel's chunked arithmetic: the output is the picked V row bit for
   bit, rows without an allowed key are zeros, nothing is NaN / Inf although every excluded key holds 0x7F7F;
2. random inputs within the per-element rounding bound of the fp64 reference, also at 1,025 and 2,049 tokens;
3. V = 1: every output within 2^-7 of 1, and from 64 tokens on as many exactly 1.0 as round-to-nearest P gives in the model (less a margin);
4. right padding to the next chunk with masked 0x7F7F tokens, and a key / value group launched alone, change no bit;
5. up to 128 tokens, heads of 64 / 128: this entry and ts_attention_short / ts_attention_gqa both lie within their own bounds of the
   same fp64 reference.  They need not agree bit for bit: P is rounded before the normalisation here and after it there;
6. the case list reaches all six instantiations."""
import ctypes as C

import pytest
import torch

import attention_bf16_common as ab
import attention_bf16_tiled_common as at
import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B = 3
shapes = pytest.mark.parametrize("hq,hkv,hd", at.HEADS, ids=lambda v: str(v))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def launch(qkv, mask, batch, S, hq, hkv, hd, causal, out):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(_ffi.load().ts_attention_flash(0, P(qkv), P(mask), batch, S, hq, hkv, hd, 1 if causal else 0, hd ** -0.5, P(out), st))


def attend(qkv, mask, hq, hkv, hd, causal):
    """The entry's answer for device tensors qkv [batch][S][...] and mask, in a guarded buffer whose margins are checked."""
    batch, S, width = qkv.shape
    assert width == (hq + 2 * hkv) * hd and qkv.dtype == BF16 and qkv.is_contiguous() and (mask is None or mask.is_contiguous())
    out = ec.guarded((batch, S, hq * hd), BF16)
    launch(qkv, mask, batch, S, hq, hkv, hd, causal, out)
    torch.cuda.synchronize()
    ec.assert_margins(out)
    return out


def dev(t):
    return None if t is None else t.cuda()


def test_the_case_list_reaches_all_six_instantiations():
    reached = {at.instantiation(hd, causal) for _, _, hd in at.HEADS + (at.WIDE_GROUP,) for causal in (False, True)}
    assert reached == at.all_instantiations() and len(reached) == 6


def selector_sweep(hq, hkv, hd, lengths, seed):
    g = ec._gen(seed, hq, hkv, hd)
    cases = keyless = 0
    for S in lengths:
        masks = at.long_masks(B, S, hd, g)
        for kind, mask in masks.items():
            for causal in (False, True):
                for pick in at.PICKS:
                    tag = (hq, hkv, hd, S, kind, causal, pick)
                    qkv, pi, has_key = at.selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, g)
                    qkv = qkv.cuda()
                    want = at.selector_want(qkv, pi, has_key, hq, hkv, hd)
                    got = attend(qkv, dev(mask), hq, hkv, hd, causal)
                    assert torch.isfinite(got).all(), (tag, "NaN / Inf: an excluded key leaked, or a maximum was not subtracted")
                    if not torch.equal(got.float(), want.float()):
                        rows = (got.float() != want.float()).view(B, S, hq, hd).any(-1).nonzero()
                        raise AssertionError((tag, f"{len(rows)} (sequence, query, head) rows are not the picked V row, first {rows[0].tolist()}",
                                              "picked key", int(pi[rows[0][0], rows[0][1]]), "has a key", bool(has_key[rows[0][0], rows[0][1]])))
                    if kind == "keyless":
                        assert not has_key[B - 1].any()
                    keyless += int((~has_key).sum())                      # (zeros in `want`: compared above)
                    cases += 1
    return cases, keyless


@shapes
def test_selectors_come_back_bit_for_bit(hq, hkv, hd, capsys):
    cases, keyless = selector_sweep(hq, hkv, hd, at.lengths(hd), 20)
    assert keyless > 0
    with capsys.disabled():
        print(f"\nts_attention_flash {hq}/{hkv} x {hd}: {cases} selector cases exact, {keyless} keyless rows exactly zero", end="")


def test_selectors_of_a_wide_group_come_back_bit_for_bit(capsys):
    """Eight query heads over one key / value head: the blocks of the group are neighbours in the grid and read the same K and V."""
    hq, hkv, hd = at.WIDE_GROUP
    C_ = at.CHUNK[hd]
    cases, keyless = selector_sweep(hq, hkv, hd, (17, C_ + 1, 3 * C_ + 17), 21)
    assert keyless > 0
    with capsys.disabled():
        print(f"\nts_attention_flash {hq}/{hkv} x {hd}: {cases} selector cases exact, {keyless} keyless rows exactly zero", end="")


@shapes
def test_random_inputs_within_the_rounding_bound(hq, hkv, hd, capsys):
    worst, worst_long, bad, keyless = 0.0, 0.0, [], 0
    for S in at.lengths(hd):
        qkv, masks = at.random_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind, mask in masks.items():
            mask = dev(mask)
            for causal in (False, True):
                tag = (hq, hkv, hd, S, kind, causal)
                want, has_key, bnd = at.bound(qkv, mask, hq, hkv, hd, causal)
                got = attend(qkv, mask, hq, hkv, hd, causal)
                assert torch.isfinite(got).all(), tag
                assert not got[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
                keyless += int((~has_key).sum())
                ratio = at.bound_ratio(got, want, has_key, bnd)
                worst = max(worst, ratio)
                if ratio > 1.0:
                    bad.append((tag, round(ratio, 3)))
    # one long sequence per length: 17 / 33 query blocks, up to 65 chunks
    for S in at.LONG_LENGTHS:
        qkv, masks = at.random_inputs(1, S, hq, hkv, hd)
        qkv, mask = qkv.cuda(), dev(masks["holes"])
        for causal in (False, True):
            want, has_key, bnd = at.bound(qkv, mask, hq, hkv, hd, causal)
            got = attend(qkv, mask, hq, hkv, hd, causal)
            assert torch.isfinite(got).all(), (hq, hkv, hd, S, causal)
            ratio = at.bound_ratio(got, want, has_key, bnd)
            worst_long = max(worst_long, ratio)
            if ratio > 1.0:
                bad.append(((hq, hkv, hd, S, "holes", causal), round(ratio, 3)))
    with capsys.disabled():
        print(f"\nts_attention_flash {hq}/{hkv} x {hd}: worst error / bound {worst:.3f} up to {max(at.lengths(hd))} tokens, {worst_long:.3f} at "
              f"1,025 / 2,049 tokens, {keyless} keyless rows exactly zero", end="")
    assert not bad, bad
    assert keyless > 0


@shapes
def test_ones_column_sums_to_one(hq, hkv, hd, capsys):
    lowest, lowest_model, bad = 1.0, 1.0, []
    for S in at.lengths(hd):
        qkv, masks = at.ones_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind, mask in masks.items():
            mask = dev(mask)
            for causal in (False, True):
                tag = (hq, hkv, hd, S, kind, causal)
                has_key = ab.allowed(mask, B, S, causal, qkv.device).any(-1)
                got = attend(qkv, mask, hq, hkv, hd, causal)
                assert torch.isfinite(got).all(), tag
                assert not got[~has_key].any(), tag
                off = (got[has_key].float() - 1.0).abs().max().item() if has_key.any() else 0.0
                assert off <= 2.0 ** -7, (tag, off)
                if S >= at.ONES_MIN_SEQ:
                    model = at.ones_share(at.emulate_online(qkv, mask, hq, hkv, hd, causal, at.CHUNK[hd]), has_key)
                    share = at.ones_share(got, has_key)
                    lowest, lowest_model = min(lowest, share), min(lowest_model, model)
                    if share < model - at.ONES_MARGIN:
                        bad.append((tag, round(share, 3), round(model, 3)))
    with capsys.disabled():
        print(f"\nts_attention_flash {hq}/{hkv} x {hd}: lowest share of outputs exactly 1.0 from {at.ONES_MIN_SEQ} tokens on {lowest:.3f} "
              f"(the model's: {lowest_model:.3f})", end="")
    assert not bad, bad


@shapes
def test_right_padding_to_the_next_chunk_changes_no_bit(hq, hkv, hd):
    """A batch at S0 tokens re-laid at the next multiple of the chunk with masked 0x7F7F tokens behind it: the first S0 rows are the
    same bits.  The extra keys' scores are discarded by a select, each adds an exact 0 to the row's sum and 0 x finite to the
    accumulators; a whole extra chunk rescales by exactly 1."""
    Cn = at.CHUNK[hd]
    for S0 in (17, Cn - 1, Cn, 2 * Cn + 1):
        qkv0, masks = at.random_inputs(B, S0, hq, hkv, hd)
        qkv0 = qkv0.cuda()
        for kind in ("none", "holes"):
            mask0 = dev(masks[kind])
            for causal in (False, True):
                base = attend(qkv0, mask0, hq, hkv, hd, causal)
                assert torch.isfinite(base).all()
                S = (S0 // Cn + 1) * Cn
                qkv, mask = at.pad_right(qkv0, S)
                if mask0 is not None:
                    mask[:, :S0] = mask0
                got = attend(qkv, mask, hq, hkv, hd, causal)[:, :S0]
                assert torch.isfinite(got).all(), (hq, hkv, hd, S0, S, kind, causal)
                assert torch.equal(got.float(), base.float()), (hq, hkv, hd, S0, S, kind, causal, (got.float() - base.float()).abs().max().item())


@pytest.mark.parametrize("hq,hkv,hd", at.HEADS + (at.WIDE_GROUP,), ids=lambda v: str(v))
def test_a_group_alone_equals_the_group_in_the_batch(hq, hkv, hd):
    """Each (sequence, key / value group) as a call of its own (B = 1, hq = per_kv, hkv = 1) gives the bits it gave inside the batch."""
    per_kv = hq // hkv
    Cn = at.CHUNK[hd]
    for S in (65, 2 * Cn + 1):
        qkv, masks = at.random_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind in ("none", "left"):
            mask = dev(masks[kind])
            for causal in (False, True):
                batch = attend(qkv, mask, hq, hkv, hd, causal).view(B, S, hkv, per_kv * hd)
                assert torch.isfinite(batch).all()
                for b in range(B):
                    for kvh in range(hkv):
                        one = attend(at.alone(qkv, b, hq, hkv, hd, kvh), None if mask is None else mask[b:b + 1].contiguous(), per_kv, 1, hd, causal)
                        assert torch.equal(one[0].float(), batch[b, :, kvh].float()), (hq, hkv, hd, S, kind, causal, b, kvh)


@pytest.mark.parametrize("entry,hq,hkv,hd", (("short", 2, 2, 64), ("gqa", 4, 2, 128)), ids=lambda v: str(v))
def test_up_to_128_tokens_both_entries_lie_within_their_own_bounds(entry, hq, hkv, hd, capsys):
    """The same inputs through ts_attention_flash and through ts_attention_short / ts_attention_gqa: each within ITS bound of the same
    fp64 reference (attention_bf16_tiled_common.bound / attention_bf16_common.bound).  Not bit for bit: this kernel rounds the
    unnormalised e to bf16 and divides the fp32 sum by l at the end, those round the normalised p."""
    lib, st = _ffi.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    worst_new = worst_old = 0.0
    differ = 0
    for S in (s for s in at.lengths(hd) if s <= 128):
        qkv, masks = at.random_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind, mask in masks.items():
            mask = dev(mask)
            for causal in ((False,) if entry == "short" else (False, True)):
                tag = (entry, S, kind, causal)
                want, has_key, bnd_new = at.bound(qkv, mask, hq, hkv, hd, causal)
                _, _, bnd_old = ab.bound(qkv, mask, hq, hkv, hd, causal)
                new = attend(qkv, mask, hq, hkv, hd, causal)
                old = ec.guarded((B, S, hq * hd), BF16)
                if entry == "short":
                    _ffi.check(lib.ts_attention_short(0, P(qkv), P(mask), B, S, hq, 64, P(old), st))
                else:
                    _ffi.check(lib.ts_attention_gqa(0, P(qkv), P(mask), B, S, hq, hkv, 128, 1 if causal else 0, P(old), st))
                torch.cuda.synchronize()
                ec.assert_margins(old)
                r_new, r_old = at.bound_ratio(new, want, has_key, bnd_new), ab.bound_ratio(old, want, has_key, bnd_old)
                assert r_new <= 1.0 and r_old <= 1.0, (tag, r_new, r_old)
                assert not new[~has_key].any() and not old[~has_key].any(), tag
                worst_new, worst_old = max(worst_new, r_new), max(worst_old, r_old)
                differ += int((new.float() != old.float()).sum())
    with capsys.disabled():
        print(f"\nup to 128 tokens, head {hd}: ts_attention_flash {worst_new:.3f} of its bound, ts_attention_{entry} {worst_old:.3f} of its own; "
              f"{differ} elements differ between them", end="")
