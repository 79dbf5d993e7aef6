"""The models behind tests/test_attention_window_gpu.py, without a GPU and without the library (tests/attention_window_common.py):
* the unmutated windowed models - the parents' arithmetic restricted to the walked chunks and, per wave, to the walked tiles - equal
  the parents' own models (attention_bf16_tiled_common.emulate_online, attention_f32_common.emulate_f32, imported, not edited) run
  with the key mask window_mask_for(q), at row q, bit for bit, on the GPU file's inputs: skipping a chunk or a tile without an allowed
  key changes no bit, which is what lets the GPU file use the pinned parent entries as its oracle; and they stay within the parents'
  bounds of the fp64 reference with the window;
* every deliberate mistake (aw.MUTANTS) fails the checks aw.CAUGHT_BY names for it, so a kernel that makes it fails on the GPU;
* the GPU file's case list skips chunks on both sides at every head size, and the probes reach the edges."""
import functools

import pytest
import torch

import attention_window_common as aw

HEADS = {hd: (hq, hkv) for hq, hkv, hd in aw.HEADS}
MODEL_PROBES = 6                                     # rows per sequence the CPU file compares (the GPU file: aw.PROBES)
entries = pytest.mark.parametrize("entry", aw.ENTRIES)


@functools.lru_cache(maxsize=None)
def case_inputs(entry, hd, S):
    hq, hkv = HEADS[hd]
    return aw.inputs(entry, aw.B, S, hq, hkv, hd)


def equiv_fails(entry, hd, S, W, kind, causal, mutate) -> bool:
    """The GPU file's check 1 with the models in the kernels' places: does any probed row differ from the parent's?"""
    hq, hkv = HEADS[hd]
    qkv, bias, masks = case_inputs(entry, hd, S)
    mask, bias = masks[kind], (bias if kind == "holes" else None)
    rep, pmasks, index = aw.parent_batch(qkv, mask, S, W, aw.probe_rows(S, W, hd, MODEL_PROBES))
    # both models on the replicated batch (torch's CPU matrix products round by the operands' shapes: the same shapes on both sides,
    # so that what differs is the model) - the windowed one with every sequence's own mask
    own = None if mask is None else torch.stack([mask[b] for b, _ in index]).contiguous()
    got = aw.emulate_w(entry, rep, own, hq, hkv, hd, causal, W, mutate, bias)
    want = aw.emulate_parent(entry, rep, pmasks, hq, hkv, hd, causal, bias)
    a, b = aw.probed(got, index, True), aw.probed(want, index, True)
    return not torch.equal(a.view(torch.int16 if entry == "flash" else torch.int32), b.view(torch.int16 if entry == "flash" else torch.int32))


def bound_ratio(entry, hd, S, W, kind, causal, mutate) -> float:
    """The GPU file's check 2 with the model in the kernel's place."""
    hq, hkv = HEADS[hd]
    qkv, bias, masks = case_inputs(entry, hd, S)
    got = aw.emulate_w(entry, qkv, masks[kind], hq, hkv, hd, causal, W, mutate, bias)
    return aw.bound_ratio(entry, got, qkv, aw.allowed_w(masks[kind], aw.B, S, causal, W), hq, hkv, hd, bias)


@entries
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_the_windowed_models_equal_the_parents_models_under_the_equivalent_key_mask(entry, hd):
    n = 0
    for S, W, kind, causal in aw.model_cases(aw.equiv_cases(hd)):
        assert not equiv_fails(entry, hd, S, W, kind, causal, None), (entry, hd, S, W, kind, causal)
        n += 1
    assert n == sum(len(aw.windows(hd, S)) for S in aw.lengths(hd))


@entries
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_the_windowed_models_stay_within_the_parents_bounds(entry, hd, capsys):
    worst = 0.0
    for S, W, kind, causal in aw.model_cases(aw.bound_cases(hd)):
        worst = max(worst, bound_ratio(entry, hd, S, W, kind, causal, None))
    with capsys.disabled():
        print(f"\n  windowed model {entry} head {hd}: worst ratio {worst:.3f} of limit {aw.limit(entry, hd)}", end="")
    # (the fp32 limit is 2 x the parent model's worst ratio: the model itself stays within half of it)
    assert 0.0 < worst <= aw.limit(entry, hd) / (1.0 if entry == "flash" else 2.0)


@entries
@pytest.mark.parametrize("mutate", aw.MUTANTS)
def test_every_mutant_fails_the_checks_named_for_it(entry, mutate):
    if entry == "tiled" and mutate in aw.FLASH_ONLY:
        with pytest.raises(AssertionError):
            aw.emulate_tiled_w(torch.zeros((1, 17, 3 * 64)), None, 1, 1, 64, False, 2, mutate)
        return
    caught = set()
    for hd in (256, 128, 64):                        # (the shortest sequences first)
        if "equiv" not in caught and any(equiv_fails(entry, hd, *case, mutate) for case in aw.model_cases(aw.equiv_cases(hd))):
            caught.add("equiv")
        if "bound" not in caught and any(bound_ratio(entry, hd, *case, mutate) > aw.limit(entry, hd) for case in aw.model_cases(aw.bound_cases(hd))):
            caught.add("bound")
        if caught == {"equiv", "bound"}:
            break
    assert caught == set(aw.CAUGHT_BY[mutate]), (entry, mutate, caught)


def test_the_case_list_skips_chunks_on_both_sides_and_the_probes_reach_the_edges():
    for hq, hkv, hd in aw.HEADS:
        C = aw.CHUNK[hd]
        assert aw.lengths(hd) == tuple(sorted({17, 65, C + 1, 2 * C + 1, 3 * C + 17, 4 * C + 65}))
        first_late = last_early = tiles_late = False
        for S, W, _, causal in aw.equiv_cases(hd):
            assert W < S and W in (1, 2, 17, 64, C, C + 1, 257)
            T = -(-S // 16)
            for qi in range(T):
                c_first, nchunk, kt_first, kt_end = aw.window_range(S, W, causal, C, qi // 4, qi % 4)
                first_late |= c_first > 0
                last_early |= not causal and c_first + nchunk < -(-S // C)
                tiles_late |= kt_first > c_first * (C // 16)
            rows = aw.probe_rows(S, W, hd)
            assert 0 in rows and S - 1 in rows and len(rows) == min(aw.PROBES, S) == len(set(rows))
        assert first_late and last_early and tiles_late, hd
        assert {(S, W) for S, W, _, _ in aw.bound_cases(hd)} == {(S, W) for S in (3 * C + 17, 4 * C + 65) for W in (17, C + 1)}
    S, W = aw.LONG
    assert (S, W) == (1025, 257) and len(aw.probe_rows(S, W, 256, 32)) == 32
    # window_mask_for: query q's window and the given mask
    m = aw.window_mask_for(torch.tensor([1, 0, 1, 1, 1, 1]), 6, 3, 2)
    assert m.tolist() == [0, 0, 1, 1, 1, 0]
