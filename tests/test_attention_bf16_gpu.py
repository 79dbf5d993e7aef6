"""The four bf16 attention kernels (kernels_attention.h: attention_short_kernel, attention_rows_kernel, attention_gqa_kernel,
attention_gqa_rows_kernel, 40 instantiations) through ts_attention_short and ts_attention_gqa, against tests/attention_bf16_common.py
(tests/test_attention_bf16_model_cpu.py shows what each check rejects).  B = 3, every length next to a 16-token tile edge up to
128, head counts that leave idle waves, reach every R of the 65 .. 128 token kernel and a second key / value head; every output
lies in a sentinel-filled buffer whose margins must come back untouched:
1. selectors - inputs whose softmax is exactly one-hot in the kernels' arithmetic: the output is the picked V row bit for bit,
   rows without an allowed key are zeros, nothing is NaN / Inf although every excluded key holds 0x7F7F;
2. random inputs within the per-element rounding bound of the fp64 reference;
3. V = 1: every output within 2^-7 of 1, and as many exactly 1.0 as round-to-nearest P gives in the model (less a margin);
4. right padding with masked 0x7F7F tokens changes no number, across T and across the <= 64 / 65 .. 128 kernel boundary;
5. a (sequence, head) or key / value group alone gives the numbers it gave inside the batch (the waves' LDS slices do not overlap);
6. at the lengths with an odd tile count, what earlier kernels left in LDS changes no number."""
import ctypes as C

import pytest
import torch

import attention_bf16_common as ab
import encoder_common as ec
from theoremsearch_amd import _ffi

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B = 3
CONFIGS = tuple(("short", H, H) for H in ab.SHORT_HEADS) + tuple(("gqa", hq, hkv) for hq, hkv in ab.GQA_HEADS)
config = pytest.mark.parametrize("entry,hq,hkv", CONFIGS, ids=lambda v: str(v))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def modes(entry):
    return (False,) if entry == "short" else (False, True)          # ts_attention_short has no causal form


def launch(entry, qkv, mask, batch, S, hq, hkv, causal, out):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "short":
        assert hq == hkv and not causal
        _ffi.check(_ffi.load().ts_attention_short(0, P(qkv), P(mask), batch, S, hq, 64, P(out), st))
    else:
        _ffi.check(_ffi.load().ts_attention_gqa(0, P(qkv), P(mask), batch, S, hq, hkv, 128, 1 if causal else 0, P(out), st))


def attend(entry, qkv, mask, hq, hkv, causal):
    """The entry's answer for device tensors qkv [batch][S][...] and mask, in a guarded buffer whose margins are checked."""
    batch, S, width = qkv.shape
    hd = ab.HEAD_DIM[entry]
    assert width == (hq + 2 * hkv) * hd and qkv.dtype == BF16 and qkv.is_contiguous() and (mask is None or mask.is_contiguous())
    out = ec.guarded((batch, S, hq * hd), BF16)
    launch(entry, qkv, mask, batch, S, hq, hkv, causal, out)
    torch.cuda.synchronize()
    ec.assert_margins(out)
    return out


def dev(t):
    return None if t is None else t.cuda()


def test_the_case_list_reaches_all_forty_instantiations():
    """From attn_short_plan / attn_gqa_plan's rules (ab.kernel_of): LENGTHS x the head configurations x causal select every
    (kernel, T, causal, R) that encoder_ops.hip instantiates."""
    reached = {ab.kernel_of(entry, S, hq, hkv, causal) for entry, hq, hkv in CONFIGS for S in ab.LENGTHS for causal in modes(entry)}
    assert reached == ab.all_instantiations() and len(reached) == 40


@config
def test_selectors_come_back_bit_for_bit(entry, hq, hkv, capsys):
    hd = ab.HEAD_DIM[entry]
    g = ec._gen(10, hq, hkv, hd)
    cases = keyless = 0
    for S in ab.LENGTHS:
        masks = ec.attention_masks(B, S, g)
        assert tuple(masks) == ec.ATTN_MASK_KINDS
        for kind, mask in masks.items():
            for causal in modes(entry):
                for pick in ab.PICKS:
                    tag = (entry, hq, hkv, S, kind, causal, pick)
                    qkv, pi, has_key = ab.selector_inputs(B, S, hq, hkv, hd, mask, causal, pick, g)
                    qkv = qkv.cuda()
                    want = ab.selector_want(qkv, pi, has_key, hq, hkv, hd)
                    got = attend(entry, qkv, dev(mask), hq, hkv, causal)
                    assert torch.isfinite(got).all(), (tag, "NaN / Inf: an excluded key leaked, or a maximum was not subtracted")
                    if not torch.equal(got.float(), want.float()):
                        rows = (got.float() != want.float()).view(B, S, hq, hd).any(-1).nonzero()
                        raise AssertionError((tag, f"{len(rows)} (sequence, query, head) rows are not the picked V row, first {rows[0].tolist()}",
                                              "picked key", int(pi[rows[0][0], rows[0][1]]), "has a key", bool(has_key[rows[0][0], rows[0][1]])))
                    if kind == "keyless":
                        assert not has_key[B - 1].any()
                    keyless += int((~has_key).sum())                      # (zeros in `want`: compared above)
                    cases += 1
    assert keyless > 0
    with capsys.disabled():
        print(f"\n{entry} {hq}/{hkv}: {cases} selector cases exact, {keyless} keyless rows exactly zero", end="")


@config
def test_random_inputs_within_the_rounding_bound(entry, hq, hkv, capsys):
    hd = ab.HEAD_DIM[entry]
    worst, bad, keyless = 0.0, [], 0
    for S in ab.LENGTHS:
        qkv, masks = ab.random_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind, mask in masks.items():
            mask = dev(mask)
            for causal in modes(entry):
                tag = (entry, hq, hkv, S, kind, causal)
                want, has_key, bnd = ab.bound(qkv, mask, hq, hkv, hd, causal)
                got = attend(entry, qkv, mask, hq, hkv, causal)
                assert torch.isfinite(got).all(), tag
                assert not got[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
                keyless += int((~has_key).sum())
                ratio = ab.bound_ratio(got, want, has_key, bnd)
                worst = max(worst, ratio)
                if ratio > 1.0:
                    bad.append((tag, round(ratio, 3)))
    with capsys.disabled():
        print(f"\n{entry} {hq}/{hkv}: worst error / bound {worst:.3f}, {keyless} keyless rows exactly zero", end="")
    assert not bad, bad
    assert keyless > 0


@config
def test_ones_column_sums_to_one(entry, hq, hkv, capsys):
    hd = ab.HEAD_DIM[entry]
    lowest, lowest_model, bad = 1.0, 1.0, []
    for S in ab.LENGTHS:
        qkv, masks = ab.ones_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind, mask in masks.items():
            mask = dev(mask)
            for causal in modes(entry):
                tag = (entry, hq, hkv, S, kind, causal)
                has_key = ab.allowed(mask, B, S, causal, qkv.device).any(-1)
                got = attend(entry, qkv, mask, hq, hkv, causal)
                assert torch.isfinite(got).all(), tag
                assert not got[~has_key].any(), tag
                off = (got[has_key].float() - 1.0).abs().max().item() if has_key.any() else 0.0
                assert off <= 2.0 ** -7, (tag, off)
                if S >= ab.ONES_MIN_SEQ:
                    model = ab.ones_share(ab.emulate(qkv, mask, hq, hkv, hd, causal), has_key)
                    share = ab.ones_share(got, has_key)
                    lowest, lowest_model = min(lowest, share), min(lowest_model, model)
                    if share < model - ab.ONES_MARGIN:
                        bad.append((tag, round(share, 3), round(model, 3)))
    with capsys.disabled():
        print(f"\n{entry} {hq}/{hkv}: lowest share of outputs exactly 1.0 from {ab.ONES_MIN_SEQ} tokens on {lowest:.3f} (the model's: {lowest_model:.3f})", end="")
    assert not bad, bad


@config
def test_right_padding_changes_no_number(entry, hq, hkv):
    """A batch at S0 tokens re-laid at S > S0 with masked 0x7F7F tokens behind it: the first S0 rows are the same numbers.  Each
    extra key tile adds an exact 0 to the row's per-lane sums of weights, and each extra 32-key step of the second product adds
    0 x finite to the accumulators; the keys of the batch keep their places inside their 32-key steps."""
    hd = ab.HEAD_DIM[entry]
    for S0 in (17, 48, 64):
        qkv0, masks = ab.random_inputs(B, S0, hq, hkv, hd)
        qkv0 = qkv0.cuda()
        for kind in ("none", "holes"):
            mask0 = dev(masks[kind])
            for causal in modes(entry):
                base = attend(entry, qkv0, mask0, hq, hkv, causal)
                assert torch.isfinite(base).all()
                for S in sorted({S0 + 1, 65, 80, 128}):
                    qkv, mask = ab.pad_right(qkv0, S)
                    if mask0 is not None:
                        mask[:, :S0] = mask0
                    assert ab.kernel_of(entry, S, hq, hkv, causal) != ab.kernel_of(entry, S0, hq, hkv, causal) or S == S0 + 1
                    got = attend(entry, qkv, mask, hq, hkv, causal)[:, :S0]
                    assert torch.isfinite(got).all(), (entry, hq, hkv, S0, S, kind, causal)
                    assert torch.equal(got.float(), base.float()), (entry, hq, hkv, S0, S, kind, causal, (got.float() - base.float()).abs().max().item())


@config
def test_alone_equals_in_the_batch(entry, hq, hkv):
    """Each (sequence, head) - for ts_attention_gqa each (sequence, key / value group) - as a call of its own (B = 1, H = 1 / hq =
    per_kv, hkv = 1: the same kernel, T and R) gives the numbers it gave inside the batch: the per-wave LDS slices (attn_wave_lds,
    attn_rows_wave_lds, attn_gqa_wave_lds, attn_gqa_rows_tile_bytes) keep the waves of a workgroup apart."""
    hd = ab.HEAD_DIM[entry]
    per_kv = hq // hkv
    for S in (33, 64, 97, 128):
        qkv, masks = ab.random_inputs(B, S, hq, hkv, hd)
        qkv = qkv.cuda()
        for kind in ("none", "left"):
            mask = dev(masks[kind])
            for causal in modes(entry):
                assert ab.kernel_of(entry, S, per_kv, 1, causal) == ab.kernel_of(entry, S, hq, hkv, causal)
                batch = attend(entry, qkv, mask, hq, hkv, causal).view(B, S, hkv, per_kv * hd)
                assert torch.isfinite(batch).all()
                for b in range(B):
                    for kvh in range(hkv):
                        one = attend(entry, ab.alone(qkv, b, hq, hkv, hd, kvh), None if mask is None else mask[b:b + 1].contiguous(),
                                     per_kv, 1, causal)
                        assert torch.equal(one[0].float(), batch[b, :, kvh].float()), (entry, hq, hkv, S, kind, causal, b, kvh)


def poison_batch(entry, hq, hkv):
    """Sequences of 128 tokens for at least 1024 workgroups of the entry's 65 .. 128 token kernel: four times the compute units."""
    if entry == "short":
        return -(-4 * 1024 // hq)
    return -(-1024 // (hkv * (hq // hkv // ab.kernel_of(entry, 128, hq, hkv)[3])))


@config
def test_what_lds_held_before_changes_no_number(entry, hq, hkv):
    """At the lengths with an odd tile count (the second product's last 32-key step is half zero-filled columns), a selector
    case directly after a call at 128 tokens that leaves the worst in LDS on every compute unit: once every element 0x7F7F
    (the V^T images hold the largest finite bf16, the P images NaN), once Q = K = 0 and V = +Inf (a stale V^T column against a
    zero P would give NaN).  A correct kernel reads nothing it did not write, so the numbers are the selector's."""
    hd = ab.HEAD_DIM[entry]
    g = ec._gen(11, hq, hkv, hd)
    nb = poison_batch(entry, hq, hkv)
    width = (hq + 2 * hkv) * hd
    big = torch.full((nb, 128, width), ab.BIG_BITS, dtype=torch.int16, device="cuda").view(BF16)
    inf = torch.zeros((nb, 128, width), dtype=BF16, device="cuda")
    inf.view(nb, 128, hq + 2 * hkv, hd)[:, :, hq + hkv:] = float("inf")
    sink = ec.guarded((nb, 128, hq * hd), BF16)
    for S in ab.ODD_TILE_LENGTHS:
        masks = ec.attention_masks(B, S, g)
        for kind in ("none", "left"):
            for causal in modes(entry):
                qkv, pi, has_key = ab.selector_inputs(B, S, hq, hkv, hd, masks[kind], causal, "random", g)
                qkv, mask = qkv.cuda(), dev(masks[kind])
                want = ab.selector_want(qkv, pi, has_key, hq, hkv, hd)
                for poison in (big, inf):
                    launch(entry, poison, None, nb, 128, hq, hkv, causal, sink)
                    got = attend(entry, qkv, mask, hq, hkv, causal)
                    ec.assert_margins(sink)
                    assert torch.isfinite(got).all() and torch.equal(got.float(), want.float()), (entry, hq, hkv, S, kind, causal, poison is big)
