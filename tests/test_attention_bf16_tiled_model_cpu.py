"""The model behind tests/test_attention_bf16_tiled_gpu.py, without a GPU and without the library
(tests/attention_bf16_tiled_common.py):
* the long selector construction has the peak, the gap and the exact-zero distance its exactness argument needs;
* the unmutated chunked online-softmax model passes every check the GPU file applies, on the GPU file's own inputs: it reproduces
  every selector bit for bit, stays within the rounding bound on the random inputs (the worst ratio is printed, also at 1,025 and
  2,049 tokens), and its ones-column outputs are 1.0;
* every deliberate mistake (at.MUTANTS) fails the checks at.CAUGHT_BY names for it, so a kernel that makes it fails on the GPU;
* the bound's rounding count and the GPU file's case list: every chunk edge, three chunks, all six instantiations."""
import functools

import pytest
import torch

import attention_bf16_tiled_common as at
import encoder_common as ec

B = 3
MODEL_HEADS = {hd: (hq, hkv) for hq, hkv, hd in at.HEADS}


def model_lengths(hd):
    """A ragged tile, a second query block, a chunk edge, a third chunk (the first buffer reused), a ragged fourth."""
    C = at.CHUNK[hd]
    return (17, 65, C + 1, 2 * C + 1, 3 * C + 17)


CASES = tuple((hd, S, causal) for hd in (64, 128, 256) for S in model_lengths(hd) for causal in (False, True))


@functools.lru_cache(maxsize=None)
def random_case(hd, S, ones, batch=B):
    hq, hkv = MODEL_HEADS[hd]
    return (at.ones_inputs if ones else at.random_inputs)(batch, S, hq, hkv, hd)


@functools.lru_cache(maxsize=None)
def reference(hd, S, kind, causal, batch=B):
    hq, hkv = MODEL_HEADS[hd]
    qkv, masks = random_case(hd, S, False, batch)
    return at.bound(qkv, masks[kind], hq, hkv, hd, causal)


@functools.lru_cache(maxsize=None)
def selector_case(hd, S, kind, causal, pick):
    hq, hkv = MODEL_HEADS[hd]
    mask = at.long_masks(B, S, hd, ec._gen(18, S, hd))[kind]
    qkv, pi, has_key = at.selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, ec._gen(19, S, hd, causal, at.PICKS.index(pick)))
    return qkv, mask, has_key, at.selector_want(qkv, pi, has_key, hq, hkv, hd)


def failing_checks(hd, S, causal, mutate):
    """The checks of the GPU file that the model with `mutate` fails at this (head size, length, causal), over the eight mask
    kinds, and the figures behind them."""
    hq, hkv = MODEL_HEADS[hd]
    C = at.CHUNK[hd]
    failed, worst, share = set(), 0.0, 1.0
    for kind in at.MASK_KINDS:
        for pick in at.PICKS:
            qkv, mask, has_key, want = selector_case(hd, S, kind, causal, pick)
            got = at.emulate_online(qkv, mask, hq, hkv, hd, causal, C, mutate=mutate)
            if not (torch.isfinite(got.float()).all() and torch.equal(got.float(), want.float())):
                failed.add("selector")
        qkv, masks = random_case(hd, S, False)
        want, has_key, bnd = reference(hd, S, kind, causal)
        got = at.emulate_online(qkv, masks[kind], hq, hkv, hd, causal, C, mutate=mutate)
        ratio = at.bound_ratio(got, want, has_key, bnd)
        worst = max(worst, ratio)
        if ratio > 1.0 or got[~has_key].any():
            failed.add("bound")
        if S >= at.ONES_MIN_SEQ:
            qkv, masks = random_case(hd, S, True)
            got = at.emulate_online(qkv, masks[kind], hq, hkv, hd, causal, C, mutate=mutate)
            if ((got.float() - 1.0).abs()[has_key] > 2.0 ** -7).any() or not torch.isfinite(got.float()).all():
                failed.add("ones")
            model = at.ones_share(at.emulate_online(qkv, masks[kind], hq, hkv, hd, causal, C), has_key)
            have = at.ones_share(got, has_key)
            share = min(share, have)
            if have < model - at.ONES_MARGIN:
                failed.add("ones")
    return failed, worst, share


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_long_selector_construction_has_the_gap_and_the_peak_it_needs(hd):
    code = at.key_codes(hd)
    peak, gap = at.selector_scores(hd)
    assert (peak, -gap, at.zero_gap(hd)) == {64: (15360, 2560, 832), 128: (30720, 5120, 1177), 256: (64512, 10752, 1664)}[hd]
    assert peak < 2 ** 24 and -gap >= at.zero_gap(hd)
    # from the codes themselves, at every length the tests use (a 512-key corner of the 4,096 x 4,096 table, and the far corner)
    for first in (0, at.CODE_KEYS - 512):
        s = code[first:first + 512].double() @ code.double().T
        own = s.gather(1, (torch.arange(512) + first)[:, None])
        assert bool((own == peak).all())
        assert float((s - own).masked_fill(s == own, float("-inf")).max()) == gap and int((s == own).sum()) == 512
    sl = torch.tensor(at.scale_log2e(hd), dtype=torch.float32)
    assert float(torch.exp2(torch.tensor(gap, dtype=torch.float32) * sl)) == 0.0
    assert float(torch.exp2(torch.tensor(-float(at.zero_gap(hd)), dtype=torch.float32) * sl)) == 0.0
    assert peak * float(sl) > 128.0                                               # overflows without the max subtraction
    assert len({tuple(r.tolist()) for r in code}) == at.CODE_KEYS and torch.equal(code.to(torch.bfloat16).float(), code)


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_unmutated_model_reproduces_every_selector(hd):
    """Every length of the GPU file, every mask kind, each pick, causal and not: bit for bit the picked V row, zeros in the rows
    without a key, nothing NaN / Inf although the excluded keys hold 0x7F7F."""
    hq, hkv = MODEL_HEADS[hd]
    keyless = 0
    for S in at.lengths(hd):
        for kind in at.MASK_KINDS:
            for causal in (False, True):
                for pick in at.PICKS:
                    qkv, mask, has_key, want = selector_case(hd, S, kind, causal, pick)
                    got = at.emulate_online(qkv, mask, hq, hkv, hd, causal, at.CHUNK[hd])
                    assert torch.isfinite(got.float()).all() and torch.equal(got.float(), want.float()), (hd, S, kind, causal, pick)
                    assert not got[~has_key].any()
                    keyless += int((~has_key).sum())
    assert keyless > 0


def test_unmutated_model_passes_every_check(capsys):
    worst = {64: 0.0, 128: 0.0, 256: 0.0}
    for hd, S, causal in CASES:
        failed, ratio, share = failing_checks(hd, S, causal, None)
        assert not failed, (hd, S, causal, failed, ratio, share)
        worst[hd] = max(worst[hd], ratio)
    with capsys.disabled():
        print("\nchunked bf16 attention model: worst error / bound " + ", ".join(f"{worst[hd]:.3f} (head {hd})" for hd in worst), end="")


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_unmutated_model_stays_within_the_bound_at_the_long_lengths(hd, capsys):
    hq, hkv = MODEL_HEADS[hd]
    worst = 0.0
    for S in at.LONG_LENGTHS:
        qkv, masks = random_case(hd, S, False, 1)
        for causal in (False, True):
            want, has_key, bnd = reference(hd, S, "holes", causal, 1)
            got = at.emulate_online(qkv, masks["holes"], hq, hkv, hd, causal, at.CHUNK[hd])
            ratio = at.bound_ratio(got, want, has_key, bnd)
            assert ratio <= 1.0, (hd, S, causal, ratio)
            worst = max(worst, ratio)
    with capsys.disabled():
        print(f"\nchunked bf16 attention model, head {hd} at 1,025 / 2,049 tokens: worst error / bound {worst:.3f}", end="")


@pytest.mark.parametrize("mutate", at.MUTANTS)
def test_every_mutant_fails_the_checks_named_for_it(mutate, capsys):
    failed, worst, share = set(), 0.0, 1.0
    per_case = {}
    for hd, S, causal in CASES:
        f, ratio, sh = failing_checks(hd, S, causal, mutate)
        per_case[(hd, S, causal)] = f
        failed |= f
        worst, share = max(worst, ratio), min(share, sh)
    with capsys.disabled():
        print(f"\n{mutate}: fails {sorted(failed)}; worst error / bound {worst:.3g}, lowest ones-column share {share:.2f}", end="")
    assert set(at.CAUGHT_BY[mutate]) <= failed, (mutate, failed)
    if mutate == "stale_buffer":                                                 # (needs a third chunk)
        assert all(bool(f) == (S > 2 * at.CHUNK[hd]) for (hd, S, causal), f in per_case.items()), per_case
    if mutate in ("causal_lt", "causal_chunk_short"):
        assert all(bool(f) == causal for (hd, S, causal), f in per_case.items()), per_case
    if mutate == "kv_head_mod":                                                  # (needs fewer key / value heads than query heads, more than one)
        assert all(bool(f) == (hd == 128) for (hd, S, causal), f in per_case.items()), per_case
    if mutate in ("other_scale", "drop_chunk_edge_key", "neg_inf_nan", "masked_in_max"):
        assert all(f for f in per_case.values()), per_case                      # no head size, length or mode hides it


def test_the_rounding_count_and_the_case_list():
    assert at.n_roundings(64, 129) == 64 + 4 + 258 + 12 + 2 and at.n_roundings(256, 2049) == 256 + 4 + 4098 + 6 * 65 + 2
    # the fp32 term stays a small part of the bound: below a tenth of the 2^-8 terms' unit at every length tested
    assert all(at.n_roundings(hd, 2049) * 2.0 ** -24 < 0.1 * 2.0 ** -8 for hd in at.CHUNK)
    for hd, C in at.CHUNK.items():
        L = at.lengths(hd)
        assert {1, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 17, 129, 257} == set(L)
        assert max(-(-S // C) for S in L) >= 3 and C * hd * 2 == 16 * 1024
        # a causal block's chunk count is a function of (block, S) alone, and the last block walks every chunk
        for S in L:
            QB = -(-S // 64)
            assert at.nchunk_of(hd, True, S, QB - 1) == at.nchunk_of(hd, False, S, 0) == -(-S // C)
            assert all(at.nchunk_of(hd, True, S, qb) == min(64 * qb + 63, S - 1) // C + 1 for qb in range(QB))
    reached = {at.instantiation(hd, causal) for _, _, hd in at.HEADS + (at.WIDE_GROUP,) for causal in (False, True)}
    assert reached == at.all_instantiations() and len(reached) == 6
