"""Cases, the walked ranges, the arithmetic models and the fp64 reference for the tests of the sliding-window attention entries
ts_attention_flash_window (attention_bf16_tiled_kernel<HD, CAUSAL, true>, theoremsearch_amd/csrc/kernels_attention_bf16_tiled.h) and
ts_attention_tiled_window (attention_f32_tiled_kernel<HD, CAUSAL, true>, kernels_attention_tiled.h):
tests/test_attn_window_plan_cpu.py, tests/test_attention_window_model_cpu.py and tests/test_attention_window_gpu.py.  Plain torch on
top of the parents' common files (imported, not edited), no library: everything here runs without a GPU.

Semantics (allowed_w): query q reads key k iff |q - k| < W, and the key mask allows k, and k <= q under causal.

What a workgroup walks (window_range, the plan's four formulas restated from their definition, not from the header's text):
with q_first = 64 qblk, q_last = min(64 qblk + 63, S - 1), T = ceil(S / 16), chunks of C keys aligned to multiples of C from key 0,
  c_first  = max(0, q_first - (W - 1)) // C          c_last = min(S - 1, q_last if causal else q_last + W - 1) // C
  kt_first = max(0, 16 qi - (W - 1)) // 16           kt_end = qi + 1 if causal else min(T, (min(16 qi + 15, S - 1) + W - 1) // 16 + 1)
for the wave of query tile qi = 4 qblk + wave (qi >= T: no tile).  A key outside the wave's tiles or the block's chunks is neither
multiplied nor allowed; in the bf16 kernel's second product a 32-key step runs when either of its two tiles is walked.

The oracle.  A chunk or tile that is skipped and one that is walked with every key excluded leave m, l, o with the same bits in both
kernels (bf16: f is exactly 0 while m = -inf and exp2(0) = 1 afterwards, every e is 0; fp32: alpha is exactly 1 when the tile maximum
is -inf, every e is 0, and o + 0 x finite V = o).  So row q of a windowed call equals, bit for bit, row q of the PARENT entry - pinned
by tests/test_attention_bf16_tiled_gpu.py and tests/test_attention_f32_gpu.py - called with the key mask window_mask_for(q): q's
window and the given mask.  The models here (emulate_flash_w, emulate_tiled_w) are the parents' models' arithmetic
(attention_bf16_tiled_common.emulate_online, attention_f32_common.emulate_f32) restricted to the walked chunks and, per wave, to the
walked tiles: a row's state moves only in a chunk its block walks and in which its wave has a tile.  `mutate` names one deliberate
mistake (MUTANTS); tests/test_attention_window_model_cpu.py shows that the unmutated models equal the parents' models under
window_mask_for, and that each mutant fails the checks CAUGHT_BY names.

All rows against fp64 (reference_w): encoder_common.attention_ref's arithmetic with allowed_w.  The bounds are the parents', with
their n_roundings(hd, S) and limits unchanged: a window only removes keys, and with them roundings."""
import torch

import attention_bf16_common as ab
import attention_bf16_tiled_common as at
import attention_f32_common as af
import encoder_common as ec

ENTRIES = ("flash", "tiled")                        # ts_attention_flash_window (bf16), ts_attention_tiled_window (fp32)
CHUNK = at.CHUNK
HEADS = ((2, 2, 64), (4, 2, 128), (3, 1, 256))
MASK_KINDS = ("none", "right", "left", "holes")
B = 2
PROBES = 16                                         # probed rows per sequence: at most 32 per case
LONG = (1025, 257)                                  # (S, W) of the long case, B = 1, once per head shape
MUTANTS = ("window_le", "window_left_only", "first_chunk_late", "last_chunk_early", "wave_first_tile_late", "step_pair_dropped",
           "window_over_mask")
FLASH_ONLY = ("step_pair_dropped",)                 # the second product's 32-key steps exist in the bf16 kernel only
# which checks of the GPU file reject each mutant (asserted by tests/test_attention_window_model_cpu.py on the GPU file's inputs):
# equiv - row q against the parent under window_mask_for(q), bit for bit; bound - every row against fp64
CAUGHT_BY = {"window_le": ("equiv", "bound"), "window_left_only": ("equiv", "bound"), "first_chunk_late": ("equiv", "bound"),
             "last_chunk_early": ("equiv", "bound"), "wave_first_tile_late": ("equiv", "bound"), "step_pair_dropped": ("equiv", "bound"),
             "window_over_mask": ("equiv", "bound")}
assert set(CAUGHT_BY) == set(MUTANTS)


# ---- the case list -------------------------------------------------------------------------------------------------------------------
def lengths(hd: int) -> tuple:
    C = CHUNK[hd]
    return tuple(sorted({17, 65, C + 1, 2 * C + 1, 3 * C + 17, 4 * C + 65}))


def windows(hd: int, S: int) -> tuple:
    C = CHUNK[hd]
    return tuple(W for W in sorted({1, 2, 17, 64, C, C + 1, 257}) if W < S)


def equiv_cases(hd: int):
    """(S, W, mask kind, causal) of the bit-for-bit sweep."""
    for S in lengths(hd):
        for W in windows(hd, S):
            for kind in MASK_KINDS:
                for causal in (False, True):
                    yield S, W, kind, causal


def bound_cases(hd: int):
    """(S, W, mask kind, causal) of the fp64 sweep."""
    C = CHUNK[hd]
    for S in (3 * C + 17, 4 * C + 65):
        for W in (17, C + 1):
            for kind in MASK_KINDS:
                for causal in (False, True):
                    yield S, W, kind, causal


def model_cases(cases):
    """The cases the CPU file runs the models on: every (S, W) of `cases` once, the mask kind and causal taken in turn."""
    seen = {}
    for S, W, kind, causal in cases:
        seen.setdefault((S, W), []).append((kind, causal))
    for i, ((S, W), rest) in enumerate(sorted(seen.items())):
        kind, causal = rest[(3 * i + 1) % len(rest)]
        yield S, W, kind, causal


def inputs(entry: str, Bn: int, S: int, hq: int, hkv: int, hd: int):
    """(qkv, bias or None, masks by kind) on the CPU, seeded by the shape: the parents' random inputs (bf16 / fp32 with a projection
    bias), the same for the GPU file and the CPU file."""
    if entry == "flash":
        qkv, masks = at.random_inputs(Bn, S, hq, hkv, hd)
        return qkv, None, {k: masks[k] for k in MASK_KINDS}
    qkv, bias, masks = af.random_inputs(Bn, S, hq, hkv, hd)
    return qkv, bias, {k: masks[k] for k in MASK_KINDS}


# ---- semantics and the walked ranges -------------------------------------------------------------------------------------------------
def allowed_w(mask, Bn: int, S: int, causal: bool, W: int, device=None) -> torch.Tensor:
    """[B][S][S] bool: query q may read key k."""
    ar = torch.arange(S, device=device)
    return ab.allowed(mask, Bn, S, causal, device) & ((ar[:, None] - ar[None, :]).abs() < W)[None]


def window_range(S: int, W: int, causal: bool, C: int, qblk: int, wave: int) -> tuple:
    """(c_first, nchunk, kt_first, kt_end): the module docstring's formulas."""
    T = -(-S // 16)
    q_first, q_last = 64 * qblk, min(64 * qblk + 63, S - 1)
    c_first = max(0, q_first - (W - 1)) // C
    c_last = min(S - 1, q_last if causal else q_last + W - 1) // C
    qi = 4 * qblk + wave
    if qi >= T:
        return c_first, c_last - c_first + 1, 0, 0
    kt_first = max(0, 16 * qi - (W - 1)) // 16
    kt_end = qi + 1 if causal else min(T, (min(16 * qi + 15, S - 1) + W - 1) // 16 + 1)
    return c_first, c_last - c_first + 1, kt_first, kt_end


def window_mask_for(mask_row, S: int, q: int, W: int) -> torch.Tensor:
    """int64 [S]: the key mask that equals query q's window and the given mask (`mask_row` [S] or None)."""
    ar = torch.arange(S)
    m = ((ar - q).abs() < W).to(torch.int64)
    return m if mask_row is None else m * (mask_row.cpu() != 0).to(torch.int64)


def walked(S: int, W: int, causal: bool, C: int, mutate=None):
    """(chunks bool [S][nch], tiles bool [S][T]): the chunks query q's block walks and the key tiles its wave multiplies, with the
    mistakes first_chunk_late (a block starts a chunk late), last_chunk_early (stops a chunk early) and wave_first_tile_late (a
    wave starts a tile late)."""
    T, nch = -(-S // 16), -(-S // C)
    chunks, tiles = torch.zeros((S, nch), dtype=torch.bool), torch.zeros((S, T), dtype=torch.bool)
    for qi in range(T):
        c_first, nchunk, kt_first, kt_end = window_range(S, W, causal, C, qi // 4, qi % 4)
        c_end = c_first + nchunk
        if mutate == "first_chunk_late":
            c_first += 1
        if mutate == "last_chunk_early":
            c_end -= 1
        if mutate == "wave_first_tile_late":
            kt_first += 1
        chunks[16 * qi:16 * qi + 16, c_first:c_end] = True
        tiles[16 * qi:16 * qi + 16, kt_first:kt_end] = True
    return chunks, tiles


def _key_allow(mask, Bn, S, causal, W, mutate, dev):
    """allowed_w with the per-key mistakes: window_le (<= for <), window_left_only (keys behind the query only are cut),
    window_over_mask (the window replaces the key mask)."""
    ar = torch.arange(S, device=dev)
    d = ar[:, None] - ar[None, :]                                                            # q - k
    if mutate == "window_le":
        win = d.abs() <= W
    elif mutate == "window_left_only":
        win = d < W
    else:
        win = d.abs() < W
    return ab.allowed(None if mutate == "window_over_mask" else mask, Bn, S, causal, dev) & win[None]


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------------------------
def emulate_flash_w(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, W: int, mutate=None) -> torch.Tensor:
    """bf16 [B][S][hq hd]: at.emulate_online's arithmetic per (query, chunk), restricted to the walked chunks and tiles.
    step_pair_dropped: a 32-key step of the second product whose first tile the wave does not walk is skipped whole - its second
    tile's keys count in l and are missing from o."""
    assert mutate is None or mutate in MUTANTS, mutate
    Bn, S, _ = qkv.shape
    dev, f32, C = qkv.device, torch.float32, CHUNK[hd]
    kvh = torch.arange(hq, device=dev) // (hq // hkv)
    x = qkv.view(Bn, S, hq + 2 * hkv, hd).float()
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv][:, :, kvh], x[:, :, hq + hkv:][:, :, kvh]
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k)
    chunks, tiles = (t.to(dev) for t in walked(S, W, causal, C, mutate))
    key_tile = torch.arange(S, device=dev) // 16
    in_tiles = tiles[:, key_tile]                                                            # [S][S]: key k lies in a tile q's wave walks
    allow = (_key_allow(mask, Bn, S, causal, W, mutate, dev) & in_tiles[None])[:, None]       # [B][1][S][S]
    in_pv = torch.ones((S, S), dtype=torch.bool, device=dev)
    if mutate == "step_pair_dropped":
        first_of_step = (key_tile // 2) * 2
        in_pv = tiles[:, first_of_step]
    sl = at.scale_log2e(hd)
    ninf, zero = torch.tensor(float("-inf"), dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev)
    m = torch.full((Bn, hq, S, 1), float("-inf"), dtype=f32, device=dev)
    l = torch.zeros((Bn, hq, S, 1), dtype=f32, device=dev)
    o = torch.zeros((Bn, hq, S, hd), dtype=f32, device=dev)
    for c in range(-(-S // C)):
        lo, hi = c * C, min(S, (c + 1) * C)
        # a row's state moves only where its block walks the chunk and its wave has a tile in it
        act = (chunks[:, c] & in_tiles[:, lo:hi].any(-1))[None, None, :, None]
        if not bool(act.any()):
            continue
        a, s = allow[..., lo:hi], sc[..., lo:hi]
        m_new = torch.maximum(m, torch.where(a, s, ninf).amax(-1, keepdim=True))
        f = torch.where(m > ninf, torch.exp2((m - m_new) * sl), zero)
        e = torch.where(a, torch.exp2((s - m_new) * sl), zero)
        p = torch.where(in_pv[:, lo:hi][None, None], e, zero).to(torch.bfloat16).float()
        l = torch.where(act, l * f + e.sum(-1, keepdim=True), l)
        o = torch.where(act, o * f + torch.einsum("bhqk,bkhd->bhqd", p, v[:, lo:hi]), o)
        m = torch.where(act, m_new, m)
    inv = torch.where(l > 0, 1.0 / l, zero)
    return (o * inv).permute(0, 2, 1, 3).to(torch.bfloat16).reshape(Bn, S, hq * hd)


def emulate_tiled_w(qkv: torch.Tensor, mask, hq: int, hkv: int, hd: int, causal: bool, W: int, mutate=None, *, bias=None) -> torch.Tensor:
    """fp32 [B][S][hq hd]: af.emulate_f32's arithmetic per (query, key tile of 16), restricted to the tiles of the walked chunks that
    the query's wave walks."""
    assert (mutate is None or mutate in MUTANTS) and mutate not in FLASH_ONLY, mutate
    Bn, S, _ = qkv.shape
    dev, f32, C = qkv.device, torch.float32, CHUNK[hd]
    kvh = torch.arange(hq, device=dev) // (hq // hkv)
    x = qkv.view(Bn, S, hq + 2 * hkv, hd)
    q, k, v = x[:, :, :hq], x[:, :, hq:hq + hkv], x[:, :, hq + hkv:]
    kb = None
    if bias is not None:
        bb = bias.to(dev).view(hq + 2 * hkv, hd)
        q, kb, v = q + bb[:hq], bb[hq:hq + hkv][kvh], v + bb[hq + hkv:]
    k, v = k[:, :, kvh], v[:, :, kvh]
    T = -(-S // 16)
    SP = 16 * T
    if SP > S:
        k = torch.cat((k, k[:, S - 1:S].expand(Bn, SP - S, hq, hd)), dim=1)
        v = torch.cat((v, torch.zeros((Bn, SP - S, hq, hd), dtype=f32, device=dev)), dim=1)
    chunks, tiles = (t.to(dev) for t in walked(S, W, causal, C, mutate))
    allow = torch.nn.functional.pad(_key_allow(mask, Bn, S, causal, W, mutate, dev), (0, SP - S))[:, None]
    sl = torch.tensor(af.scale_log2e(hd), dtype=f32, device=dev)
    ninf, zero, one = (torch.tensor(c, dtype=f32, device=dev) for c in (float("-inf"), 0.0, 1.0))
    m = torch.full((Bn, hq, S, 1), float("-inf"), dtype=f32, device=dev)
    l = torch.zeros((Bn, hq, S, 1), dtype=f32, device=dev)
    o = torch.zeros((Bn, hq, S, hd), dtype=f32, device=dev)
    for kj in range(T):
        act = (tiles[:, kj] & chunks[:, 16 * kj // C])[None, None, :, None]
        if not bool(act.any()):
            continue
        lo, hi = 16 * kj, 16 * kj + 16
        kt = k[:, lo:hi] if kb is None else k[:, lo:hi] + kb
        s = torch.einsum("bqhd,bkhd->bhqk", q, kt)
        a = allow[..., lo:hi]
        m_new = torch.maximum(m, torch.where(a, s, ninf).amax(-1, keepdim=True))
        alpha = torch.where(m_new > ninf, torch.exp2((m - m_new) * sl), one)
        e = torch.where(a, torch.exp2((s - m_new) * sl), zero)
        l = torch.where(act, l * alpha + e.sum(-1, keepdim=True), l)
        o = torch.where(act, o * alpha + torch.einsum("bhqk,bkhd->bhqd", e, v[:, lo:hi]), o)
        m = torch.where(act, m_new, m)
    inv = torch.where(l > 0, 1.0 / l, zero)
    return (o * inv).permute(0, 2, 1, 3).reshape(Bn, S, hq * hd).contiguous()


def emulate_w(entry: str, qkv, mask, hq, hkv, hd, causal, W, mutate=None, bias=None):
    if entry == "flash":
        return emulate_flash_w(qkv, mask, hq, hkv, hd, causal, W, mutate)
    return emulate_tiled_w(qkv, mask, hq, hkv, hd, causal, W, mutate, bias=bias)


def emulate_parent(entry: str, qkv, mask, hq, hkv, hd, causal, bias=None):
    """The parents' own models, unwindowed."""
    if entry == "flash":
        return at.emulate_online(qkv, mask, hq, hkv, hd, causal, CHUNK[hd])
    return af.emulate_f32(qkv, mask, hq, hkv, hd, causal, "tiled", bias=bias)


# ---- the probes of the bit-for-bit check ---------------------------------------------------------------------------------------------------
def probe_rows(S: int, W: int, hd: int, n: int = PROBES) -> list:
    """At most n rows of a sequence: both ends, rows whose window edge q +- (W - 1) or q +- W falls on a chunk, 64-query-block or tile
    edge (position p with p % E in (0, E - 1); the coarser edges first, spread over the sequence), then random rows."""
    rows = [0, S - 1]
    for E in (CHUNK[hd], 64, 16):
        cand = []
        for p in [e + d for e in range(0, S + E, E) for d in (-1, 0)]:
            cand += [p - (W - 1), p + (W - 1), p - W, p + W]
        cand = sorted({q for q in cand if 0 <= q < S} - set(rows))
        take = max(1, (n - 4) // 3)
        step = max(1, len(cand) // take)
        rows += cand[::step][:take]
    g = ec._gen(31, S, W, hd)
    while len(rows) < min(n, S):
        q = int(torch.randint(0, S, (1,), generator=g))
        if q not in rows:
            rows.append(q)
    return sorted(rows[:n])


def parent_batch(qkv: torch.Tensor, mask, S: int, W: int, rows: list):
    """(qkv [B len(rows)][S][...], mask int64 [B len(rows)][S], index): every sequence of the batch replicated once per probed row,
    with the key mask window_mask_for(q); row index[i] = (b, q) of the windowed call is row q of sequence i here."""
    Bn = qkv.shape[0]
    index = [(b, q) for b in range(Bn) for q in rows]
    rep = torch.stack([qkv[b] for b, _ in index]).contiguous()
    masks = torch.stack([window_mask_for(None if mask is None else mask[b], S, q, W) for b, q in index]).contiguous()
    return rep, masks, index


def probed(out: torch.Tensor, index: list, parent: bool) -> torch.Tensor:
    """The probed rows [len(index)][width] of a windowed call's output (parent=False) or of the replicated parent call's."""
    if parent:
        return torch.stack([out[i, q] for i, (_, q) in enumerate(index)])
    return torch.stack([out[b, q] for b, q in index])


# ---- all rows against fp64 ---------------------------------------------------------------------------------------------------------------------
def reference_w(qkv, allow: torch.Tensor, hq: int, hkv: int, hd: int, bias=None):
    """(want fp64 [B][S][hq hd], has_key bool [B][S], A fp64): ec.attention_ref's arithmetic with `allow` [B][S][S] in the place of its
    own mask, and the same with |V| in V's place (A = sum_k p_k |v_kd|)."""
    if bias is not None:
        qkv = qkv + bias.to(qkv.device)
    Bn, S, _ = qkv.shape
    q = qkv[..., :hq * hd].view(Bn, S, hq, hd).double()
    k = qkv[..., hq * hd:(hq + hkv) * hd].view(Bn, S, hkv, hd).double().repeat_interleave(hq // hkv, dim=2)
    v = qkv[..., (hq + hkv) * hd:].view(Bn, S, hkv, hd).double().repeat_interleave(hq // hkv, dim=2)
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) * hd ** -0.5
    allow = allow[:, None]
    has_key = allow.any(dim=-1, keepdim=True)
    sc = sc.masked_fill(~allow, float("-inf"))
    p = torch.softmax(sc.masked_fill(~has_key, 0.0), dim=-1)
    p = torch.where(has_key & allow, p, torch.zeros_like(p))
    want = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(Bn, S, hq * hd)
    A = torch.einsum("bhqk,bkhd->bqhd", p, v.abs()).reshape(Bn, S, hq * hd)
    return want, has_key[:, 0, :, 0], A


def bound_ratio(entry: str, got, qkv, allow, hq: int, hkv: int, hd: int, bias=None) -> float:
    """The worst |got - want| over the parent's bound (flash: at.bound's 2^-8 (A + |want|) + n_roundings(hd, S) 2^-24 A, limit 1;
    tiled: af.unit's 2^-24 (A + |want|), limit af.LIMIT[hd]) over the rows with a key; rows without one must be zeros."""
    S = qkv.shape[1]
    want, has_key, A = reference_w(qkv, allow, hq, hkv, hd, bias)
    if entry == "flash":
        u = ec.UNIT[torch.bfloat16]
        bnd = u * (A + want.abs()) + at.n_roundings(hd, S) * ec.UNIT[torch.float32] * A
    else:
        bnd = ec.UNIT[torch.float32] * (A + want.abs())
    if bool((~has_key).any()) and not bool((got[~has_key] == 0).all()):
        return 1e30
    return ab.bound_ratio(got, want, has_key, bnd)


def limit(entry: str, hd: int) -> float:
    return 1.0 if entry == "flash" else af.LIMIT[hd]
