"""The model behind tests/test_attention_f32_gpu.py, without a GPU and without the library (tests/attention_f32_common.py):
* the fp32 selector construction has what its exactness argument needs: integer scores exact in any order, a gap beyond the
  exact-zero distance, excluded keys whose scores overflow, V that no bf16 holds;
* the unmutated tile-wise running-softmax model reproduces every selector and every V-bias selector of the GPU file's case list bit
  for bit, zeros in the keyless rows, nothing NaN / Inf, pieces = split_ref;
* the model's worst r = |got - fp64| / (2^-24 (A + |want|)) over the GPU file's random and ones-column inputs is recomputed, printed
  next to af.LIMIT and held to LIMIT / 2 >= worst >= LIMIT / 4;
* every deliberate mistake (af.MUTANTS) fails the checks af.CAUGHT_BY names for it - printed per mutant - so a kernel that makes it
  fails on the GPU; h % hkv for h // (hq / hkv) is caught at all three head sizes;
* the case list reaches all twelve instantiations, 1 / 2 / 3 / 4 waves of attention_f32_kernel and its causal far-end rounds."""
import functools

import pytest
import torch

import attention_f32_common as af
import encoder_common as ec

MODEL_HEADS = {hd: (hq, hkv) for hq, hkv, hd in af.HEADS}


def mutant_lengths(hd):
    """A ragged tile, a chunk edge, a third chunk (the first buffer reused) and a ragged fourth - all lengths of the GPU file."""
    C = af.CHUNK[hd]
    return (17, C + 1, 2 * C + 1, 3 * C + 17)


MUTANT_CASES = tuple((hd, S, causal) for hd in (64, 128, 256) for S in mutant_lengths(hd) for causal in (False, True))


def entry_for(hd, S, mutate):
    """Mutants run as the entry that reaches the length; the chunk-staging ones exist for `tiled` only."""
    return "tiled" if mutate in af.TILED_ONLY or S > af.FLOAT_MAX_SEQ[hd] else "float"


@functools.lru_cache(maxsize=None)
def random_case(hd, Bn, S):
    hq, hkv = MODEL_HEADS[hd]
    return af.random_inputs(Bn, S, hq, hkv, hd)


@functools.lru_cache(maxsize=None)
def reference(hd, Bn, S, kind, causal):
    hq, hkv = MODEL_HEADS[hd]
    qkv, bias, masks = random_case(hd, Bn, S)
    return af.unit(af.masked(qkv, masks[kind], hq, hkv, hd), masks[kind], hq, hkv, hd, causal, bias=bias)


def selector_ok(got, want, has_key):
    return bool(torch.isfinite(got).all()) and ec.same_bits(got, want) and not got[~has_key].any() \
        and ec.same_bits(ec.split_ref(got.view(-1, got.shape[-1])), ec.split_ref(want.view(-1, want.shape[-1])))


def fails(check, hd, S, causal, mutate):
    """Whether the model with `mutate` fails `check` of the GPU file at this (head size, length, causal) under some mask kind, and
    the worst r seen (bound, ones).  Stops at the first failing kind."""
    hq, hkv = MODEL_HEADS[hd]
    entry = entry_for(hd, S, mutate)
    worst = 0.0
    for kind in af.MASK_KINDS:
        if check in ("selector", "vbias_selector", "poison"):
            for pick in af.PICKS:
                qkv, bias, mask, has_key, want = af.selector_case(hq, hkv, hd, S, kind, causal, pick, vbias=check == "vbias_selector")
                got = af.emulate_f32(qkv, mask, hq, hkv, hd, causal, entry, mutate, bias=bias, tail=float("inf") if check == "poison" else 1.0)
                if not selector_ok(got, want, has_key):
                    return True, worst
        else:
            qkv, bias, masks = random_case(hd, af.B, S)
            mask = masks[kind]
            if check == "bound":
                want, has_key, u = reference(hd, af.B, S, kind, causal)
                got = af.emulate_f32(af.masked(qkv, mask, hq, hkv, hd), mask, hq, hkv, hd, causal, entry, mutate, bias=bias)
            else:
                x = af.masked(qkv, mask, hq, hkv, hd, ones=True)
                want, has_key, u = af.unit(x, mask, hq, hkv, hd, causal, ones=True)
                got = af.emulate_f32(x, mask, hq, hkv, hd, causal, entry, mutate)
            worst = max(worst, af.worst_r(got, want, has_key, u))
            if worst > af.LIMIT[hd] or got[~has_key].any():
                return True, worst
    return False, worst


@functools.lru_cache(maxsize=None)
def model_sweep(hd):
    """The unmutated model over the GPU file's random and ones-column inputs at this head size: (worst r random, worst r ones,
    where the worst was, keyless rows seen)."""
    hq, hkv = MODEL_HEADS[hd]
    worst, worst_ones, at_, keyless = 0.0, 0.0, None, 0
    for Bn, S, kind in af.bound_cases("tiled", hq, hkv, hd):
        qkv, bias, masks = random_case(hd, Bn, S)
        mask = masks[kind]
        x, x1 = af.masked(qkv, mask, hq, hkv, hd), af.masked(qkv, mask, hq, hkv, hd, ones=True)
        for causal in (False, True):
            want, has_key, u = af.unit(x, mask, hq, hkv, hd, causal, bias=bias)
            got = af.emulate_f32(x, mask, hq, hkv, hd, causal, "tiled", bias=bias)
            assert torch.isfinite(got).all() and not got[~has_key].any(), (hd, Bn, S, kind, causal)
            r = af.worst_r(got, want, has_key, u)
            if r > worst:
                worst, at_ = r, (Bn, S, kind, causal)
            want, has_key, u = af.unit(x1, mask, hq, hkv, hd, causal, ones=True)
            got = af.emulate_f32(x1, mask, hq, hkv, hd, causal, "tiled")
            assert torch.isfinite(got).all() and not got[~has_key].any(), (hd, Bn, S, kind, causal)
            worst_ones = max(worst_ones, af.worst_r(got, want, has_key, u))
            keyless += int((~has_key).sum())
    return worst, worst_ones, at_, keyless


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_selector_construction_has_what_its_exactness_needs(hd):
    code = af.key_codes(hd)
    peak, gap = af.selector_scores(hd)
    assert (peak, -gap, af.zero_gap(hd)) == {64: (15360, 2560, 832), 128: (30720, 5120, 1177), 256: (64512, 10752, 1664)}[hd]
    # every product is +-256 or 0, so every partial sum of any order is an integer of at most 256 hd < 2^24: exact in fp32
    assert set(code.unique().tolist()) <= {-16.0, 0.0, 16.0} and 256 * hd < 2 ** 24
    s32 = code[:600] @ code[:600].T
    assert torch.equal(s32.double(), code[:600].double() @ code[:600].double().T)
    assert torch.equal(s32, (code[:600].flip(-1) @ code[:600].flip(-1).T))                  # another order, the same bits
    off = s32 - torch.diag(torch.full((600,), float("inf")))
    assert float(s32.diagonal().min()) == float(s32.diagonal().max()) == peak and float(off.max()) == peak + gap
    assert -gap > af.zero_gap(hd)
    sl = torch.tensor(af.scale_log2e(hd), dtype=torch.float32)
    assert float(torch.exp2(torch.tensor(gap, dtype=torch.float32) * sl)) == 0.0
    assert float(torch.exp2(torch.tensor(-float(af.zero_gap(hd)), dtype=torch.float32) * sl)) == 0.0
    assert peak * float(sl) > 128.0                                                          # overflows without the max subtraction
    # an excluded key: the largest bf16-representable fp32, finite, and its score against a code overflows
    big = af.big()
    assert float(big) == 3.3895313892515355e38 and torch.isfinite(big) and not torch.isfinite(big * 16.0 + big * 16.0)
    assert float(big + 1.0e30) == float(big) and torch.isfinite(big + 4.0)                  # V's bias does not move it, let alone to Inf
    # V of a selector keeps mantissa bits no bf16 has
    qkv, _, _, _, _ = af.selector_case(*MODEL_HEADS[hd], hd, 17, "none", False, "first")
    v = qkv.view(af.B, 17, -1, hd)[:, :, 6:]
    assert float((v.bfloat16().float() != v).double().mean()) > 0.99


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_unmutated_model_reproduces_every_selector_of_the_case_list(hd, capsys):
    """Every length, mask kind, pick, causal and not, with and without V's bias: bit for bit the picked V row (plus bias_v), zeros in
    the rows without a key, pieces = split_ref, nothing NaN / Inf although the excluded keys' scores overflow.  `float`'s lengths
    are a subset of `tiled`'s and without a mutant the entry changes nothing in the model (asserted), so one run serves both."""
    hq, hkv = MODEL_HEADS[hd]
    assert set(af.lengths("float", hd)) < set(af.lengths("tiled", hd))
    cases = keyless = 0
    for S in af.lengths("tiled", hd):
        for kind in af.MASK_KINDS:
            for causal in (False, True):
                for pick in af.PICKS:
                    for vbias in (False, True):
                        qkv, bias, mask, has_key, want = af.selector_case(hq, hkv, hd, S, kind, causal, pick, vbias)
                        got = af.emulate_f32(qkv, mask, hq, hkv, hd, causal, "tiled", bias=bias)
                        assert selector_ok(got, want, has_key), (hd, S, kind, causal, pick, vbias)
                        if S == 17:
                            assert ec.same_bits(got, af.emulate_f32(qkv, mask, hq, hkv, hd, causal, "float", bias=bias))
                        keyless += int((~has_key).sum())
                        cases += 1
    assert keyless > 0
    with capsys.disabled():
        print(f"\nfp32 attention model, head {hd}: {cases} selector cases exact, {keyless} keyless rows exactly zero", end="")


def test_unmutated_model_reproduces_the_wide_group_selectors():
    hq, hkv, hd = af.WIDE_GROUP
    for S in (17, af.CHUNK[hd] + 1):
        for kind in ("holes", "keyless"):
            for causal in (False, True):
                for vbias in (False, True):
                    qkv, bias, mask, has_key, want = af.selector_case(hq, hkv, hd, S, kind, causal, "random", vbias)
                    assert selector_ok(af.emulate_f32(qkv, mask, hq, hkv, hd, causal, "float", bias=bias), want, has_key)


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_the_limit_table_is_twice_the_models_worst_r(hd, capsys):
    worst, worst_ones, where, keyless = model_sweep(hd)
    top = max(worst, worst_ones)
    with capsys.disabled():
        print(f"\nfp32 attention model, head {hd}: worst r {worst:.2f} on the random inputs at (B, S, mask, causal) = {where}, {worst_ones:.2f} on "
              f"the ones column; table LIMIT = {af.LIMIT[hd]:g} (MODEL_WORST {af.MODEL_WORST[hd]:g}): LIMIT / worst = {af.LIMIT[hd] / top:.2f}", end="")
    assert keyless > 0
    assert af.LIMIT[hd] / 2 >= top >= af.LIMIT[hd] / 4, (hd, top, af.LIMIT[hd])
    assert af.LIMIT[hd] >= 2 * af.MODEL_WORST[hd] > af.LIMIT[hd] - 5 and af.LIMIT[hd] % 5 == 0, "LIMIT is 2 x MODEL_WORST, rounded up to a multiple of 5"

def test_unmutated_model_passes_every_check():
    for hd, S, causal in MUTANT_CASES:
        for check in ("selector", "vbias_selector", "bound", "ones", "poison"):
            failed, worst = fails(check, hd, S, causal, None)
            assert not failed, (hd, S, causal, check, worst)
    # a finite leftover past S changes nothing at all (0 x finite = 0): only what the poisoning launch leaves shows the mistake
    for hd, S, causal in MUTANT_CASES:
        for check in ("selector", "bound"):
            assert not fails(check, hd, S, causal, "vt_tail_not_zero")[0], (hd, S, causal, check)


@pytest.mark.parametrize("mutate", af.MUTANTS)
def test_every_mutant_fails_the_checks_named_for_it(mutate, capsys):
    per_check, worst = {}, 0.0
    for check in af.CAUGHT_BY[mutate]:
        per_case = {}
        for hd, S, causal in MUTANT_CASES:
            per_case[(hd, S, causal)], r = fails(check, hd, S, causal, mutate)
            worst = max(worst, r)
        per_check[check] = per_case
        assert any(per_case.values()), (mutate, check)
        heads = {hd for (hd, S, causal), f in per_case.items() if f}
        assert heads == {64, 128, 256}, (mutate, check, "no head size may hide it", heads)
        if mutate == "stale_buffer":                                               # (needs a third chunk)
            assert all(f == (S > 2 * af.CHUNK[hd]) for (hd, S, causal), f in per_case.items()), per_case
        if mutate in ("causal_lt", "causal_chunk_short"):
            assert all(f == causal for (hd, S, causal), f in per_case.items()), per_case
        if mutate in ("other_scale", "drop_last_key", "drop_chunk_edge_key", "alpha_nan_at_neg_inf", "masked_in_max", "kv_head_mod", "v_bias_dropped",
                      "vt_tail_not_zero"):
            assert all(per_case.values()), (mutate, check, per_case)               # no head size, length or mode hides it
        if mutate == "k_bias_added_twice":                                         # (every length here has a second tile)
            assert all(per_case.values()), (mutate, check, per_case)
    with capsys.disabled():
        print(f"\n{mutate}: rejected by " + ", ".join(f"{c} ({sum(p.values())} of {len(p)} cases)" for c, p in per_check.items())
              + (f"; worst r {worst:.3g}" if worst else ""), end="")


def test_kv_head_mod_is_caught_at_all_three_head_sizes():
    """h % hkv for h // (hq / hkv): with (4, 2, hd) query heads 1 and 2 read the other key / value head.  The earlier shapes (2, 2, 64)
    and (3, 1, 256) cannot tell the two apart."""
    for hq, hkv, hd in ((2, 2, 64), (3, 1, 256)):
        h = torch.arange(hq)
        assert torch.equal(h % hkv, h // (hq // hkv))
    for hd in (64, 128, 256):
        hq, hkv = MODEL_HEADS[hd]
        h = torch.arange(hq)
        assert 1 < hkv < hq and not torch.equal(h % hkv, h // (hq // hkv))
        for check in ("selector", "vbias_selector", "bound"):
            assert all(fails(check, hd, S, causal, "kv_head_mod")[0] for S in mutant_lengths(hd) for causal in (False, True)), (hd, check)
    hq, hkv, hd = af.WIDE_GROUP
    assert torch.equal(torch.arange(hq) % hkv, torch.arange(hq) // (hq // hkv))          # (one key / value head: nothing to confuse)


def test_the_case_list():
    assert af.reached_instantiations() == af.all_instantiations() and len(af.all_instantiations()) == 12
    assert all(1 < hkv < hq for hq, hkv, _ in af.HEADS) and {hd for _, _, hd in af.HEADS} == {64, 128, 256} and af.WIDE_GROUP == (8, 1, 128)
    for hd, C in af.CHUNK.items():
        lim = af.FLOAT_MAX_SEQ[hd]
        Lt, Lf = af.lengths("tiled", hd), af.lengths("float", hd)
        assert {1, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 17, lim, lim + 1} <= set(Lt)
        assert max(Lf) == lim and lim + 1 not in Lf and max(-(-S // C) for S in Lt) >= 3 and max(Lt) <= 513
        assert {af.float_waves(S) for S in Lf} == {1, 2, 3, 4}
        # causal: a ragged and a full round from the far end (T = 5, 8); heads of 64 / 128 also a third round (T > 8)
        assert {5, 8} <= {-(-S // 16) for S in Lf} and (hd == 256 or any(-(-S // 16) > 8 for S in Lf))
        assert [(Bn, S) for Bn, S, _ in af.bound_cases("tiled", 4, 2, hd)][-2:] == [(1, 1025), (1, 2049)]
        assert all(Bn == af.B and S <= lim for Bn, S, _ in af.bound_cases("float", 4, 2, hd))
    assert af.MASK_KINDS == ec.ATTN_MASK_KINDS + ("chunk_of_padding", "one_key")
