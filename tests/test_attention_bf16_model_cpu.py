"""The model behind tests/test_attention_bf16_gpu.py, without a GPU and without the library (tests/attention_bf16_common.py):
* the selector construction has the score gap and the peak score its exactness argument needs - from the construction itself;
* the unmutated emulation of the kernels' arithmetic passes every check the GPU file applies, on the GPU file's own inputs: it
  reproduces every selector bit for bit, stays within the rounding bound on the random inputs, and its ones-column outputs are 1.0;
* every deliberate mistake (ab.MUTANTS) fails the checks ab.CAUGHT_BY names for it, so a kernel that makes it fails on the GPU;
* the launch rules re-stated in Python reach all 40 kernel instantiations over the GPU file's lengths and head counts."""
import functools

import pytest
import torch

import attention_bf16_common as ab
import encoder_common as ec

B = 3
MODEL_LENGTHS = (17, 64, 65, 128)
# one head configuration per head size: ts_attention_short's layout is hq = hkv; 4 / 2 has two groups of two query heads
MODEL_HEADS = {64: (5, 5), 128: (4, 2)}
CASES = tuple((hd, S, causal) for hd in (64, 128) for S in MODEL_LENGTHS for causal in (False, True))


@functools.lru_cache(maxsize=None)
def random_case(hd, S, ones):
    hq, hkv = MODEL_HEADS[hd]
    return (ab.ones_inputs if ones else ab.random_inputs)(B, S, hq, hkv, hd)


@functools.lru_cache(maxsize=None)
def reference(hd, S, kind, causal):
    hq, hkv = MODEL_HEADS[hd]
    qkv, masks = random_case(hd, S, False)
    return ab.bound(qkv, masks[kind], hq, hkv, hd, causal)


@functools.lru_cache(maxsize=None)
def selector_case(hd, S, kind, causal, pick):
    hq, hkv = MODEL_HEADS[hd]
    mask = ec.attention_masks(B, S, ec._gen(8, S, hd))[kind]
    qkv, pi, has_key = ab.selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, ec._gen(9, S, hd, causal, ab.PICKS.index(pick)))
    return qkv, mask, has_key, ab.selector_want(qkv, pi, has_key, hq, hkv, hd)


def failing_checks(hd, S, causal, mutate):
    """The checks of the GPU file that the emulation with `mutate` fails at this (head size, length, causal), over the six mask
    kinds, and the figures behind them."""
    hq, hkv = MODEL_HEADS[hd]
    failed, worst, share = set(), 0.0, 1.0
    for kind in ec.ATTN_MASK_KINDS:
        for pick in ab.PICKS:
            qkv, mask, has_key, want = selector_case(hd, S, kind, causal, pick)
            got = ab.emulate(qkv, mask, hq, hkv, hd, causal, mutate=mutate)
            if not (torch.isfinite(got.float()).all() and torch.equal(got.float(), want.float())):
                failed.add("selector")
        qkv, masks = random_case(hd, S, False)
        want, has_key, bnd = reference(hd, S, kind, causal)
        got = ab.emulate(qkv, masks[kind], hq, hkv, hd, causal, mutate=mutate)
        ratio = ab.bound_ratio(got, want, has_key, bnd)
        worst = max(worst, ratio)
        if ratio > 1.0 or got[~has_key].any():
            failed.add("bound")
        qkv, masks = random_case(hd, S, True)
        got = ab.emulate(qkv, masks[kind], hq, hkv, hd, causal, mutate=mutate)
        if ((got.float() - 1.0).abs()[has_key] > 2.0 ** -7).any() or not torch.isfinite(got.float()).all():
            failed.add("ones")
        if S >= ab.ONES_MIN_SEQ:
            model = ab.ones_share(ab.emulate(qkv, masks[kind], hq, hkv, hd, causal), has_key)
            have = ab.ones_share(got, has_key)
            share = min(share, have)
            if have < model - ab.ONES_MARGIN:
                failed.add("ones")
    return failed, worst, share


@pytest.mark.parametrize("hd", (64, 128))
def test_selector_construction_has_the_gap_and_the_peak_it_needs(hd):
    """From key_codes itself: a key's score against its own code is 64 (hd // 7) 7 (4032 / 8064: exp2f overflows without the max
    subtraction - the largest fp32 exponent is 128), the closest wrong key scores 2 * 64 (hd // 7) lower (1152 / 2304), and that is
    further than the distance at which exp2f of the scaled difference is exactly 0 (832 / 1177): in torch's fp32 exp2 as well."""
    peak, gap = ab.selector_scores(hd)
    reps = hd // ab.CODE_BITS
    assert peak == ab.CODE_VALUE ** 2 * reps * ab.CODE_BITS and gap == -2 * ab.CODE_VALUE ** 2 * reps
    assert peak < 2 ** 24                                                        # integers this small are exact in fp32
    assert ab.zero_gap(hd) == {64: 832, 128: 1177}[hd] and -gap >= ab.zero_gap(hd)
    sl = torch.tensor(ab.scale_log2e(hd), dtype=torch.float32)
    assert float(torch.exp2(torch.tensor(gap, dtype=torch.float32) * sl)) == 0.0
    assert float(torch.exp2(torch.tensor(-float(ab.zero_gap(hd)), dtype=torch.float32) * sl)) == 0.0
    assert peak * float(sl) > 128.0
    code = ab.key_codes(hd)
    assert len({tuple(r.tolist()) for r in code}) == 128 and torch.equal(code.to(torch.bfloat16).float(), code)
    big = torch.tensor([ab.BIG_BITS], dtype=torch.int16).view(torch.bfloat16)
    assert torch.isfinite(big.float()).all() and torch.isinf((big.float() * (1 + 2.0 ** -7)).to(torch.bfloat16)).all()


@pytest.mark.parametrize("hd", (64, 128))
def test_unmutated_emulation_reproduces_every_selector(hd):
    """Every length of the GPU file, every mask kind, each pick, causal and not: bit for bit the picked V row, zeros in the
    rows without a key, nothing NaN / Inf although the excluded keys hold 0x7F7F."""
    hq, hkv = MODEL_HEADS[hd]
    keyless = 0
    for S in ab.LENGTHS:
        for kind in ec.ATTN_MASK_KINDS:
            for causal in (False, True):
                for pick in ab.PICKS:
                    qkv, mask, has_key, want = selector_case(hd, S, kind, causal, pick)
                    got = ab.emulate(qkv, mask, hq, hkv, hd, causal)
                    assert torch.isfinite(got.float()).all() and torch.equal(got.float(), want.float()), (hd, S, kind, causal, pick)
                    assert not got[~has_key].any()
                    keyless += int((~has_key).sum())
    assert keyless > 0


def test_unmutated_emulation_passes_every_check(capsys):
    worst = {64: 0.0, 128: 0.0}
    for hd, S, causal in CASES:
        failed, ratio, share = failing_checks(hd, S, causal, None)
        assert not failed, (hd, S, causal, failed, ratio, share)
        worst[hd] = max(worst[hd], ratio)
    with capsys.disabled():
        print(f"\nbf16 attention model: worst error / bound {worst[64]:.3f} (head 64), {worst[128]:.3f} (head 128)", end="")


@pytest.mark.parametrize("mutate", ab.MUTANTS)
def test_every_mutant_fails_the_checks_named_for_it(mutate, capsys):
    """Over the model's cases (the mistakes that need it under causal / with fewer key / value heads than query heads only
    there), the checks ab.CAUGHT_BY names all fail.  truncate_p against the bound is the closest call: 1.16 - 1.27 of it."""
    failed, worst, share = set(), 0.0, 1.0
    per_case = {}
    for hd, S, causal in CASES:
        f, ratio, sh = failing_checks(hd, S, causal, mutate)
        per_case[(hd, S, causal)] = f
        failed |= f
        worst, share = max(worst, ratio), min(share, sh)
    with capsys.disabled():
        print(f"\n{mutate}: fails {sorted(failed)}; worst error / bound {worst:.3g}, lowest ones-column share {share:.2f}", end="")
    assert set(ab.CAUGHT_BY[mutate]) <= failed, (mutate, failed)
    if mutate == "truncate_p":
        # the rounding direction of P shows at every length from ONES_MIN_SEQ on, for both head sizes, causal or not
        assert all("ones" in f for (hd, S, causal), f in per_case.items() if S >= ab.ONES_MIN_SEQ), per_case
    if mutate in ("other_scale", "swap_key_pair", "drop_last_key"):
        assert all(f for f in per_case.values()), per_case                      # no head size, length or mode hides it
    if mutate == "stale_pad":                                                    # (a multiple of 32 has no such column)
        assert all(bool(f) == (S % 32 != 0) for (hd, S, causal), f in per_case.items()), per_case
    if mutate == "kv_head_mod":
        assert all(f for (hd, S, causal), f in per_case.items() if hd == 128), per_case


def test_the_case_list_reaches_all_forty_instantiations():
    assert ab.reached_instantiations() == ab.all_instantiations()
    assert {ab.kernel_of("gqa", 128, hq, hkv, False)[3] for hq, hkv in ab.GQA_HEADS} == {1, 2, 4}
    # a full tile, one token short of it and one over the one before, for every T
    assert {T: sorted(S for S in ab.LENGTHS if -(-S // 16) == T) for T in range(1, 9)} == \
        {T: sorted({max(1, 16 * T - 15), 16 * T - 1, 16 * T}) for T in range(1, 9)}
    assert ab.ODD_TILE_LENGTHS == (1, 15, 16, 33, 47, 48, 65, 79, 80, 97, 111, 112)
