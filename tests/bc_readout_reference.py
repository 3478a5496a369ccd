"""The probe read-outs of one call (csrc/bc_readout.hip: k_bc_readout, one launch per chunk) restated in numpy by chunk, tile and
lane, for the tests of the sizes the read-outs accept: the cases that test_gpu_bc_readout.py runs on the device, and the WRONG
rules those cases are built to see, which test_bc_readout.py shows they do.  Test infrastructure; it never imports the package.

  TILE_CASES, list_case(), probe_heads()   the cases: rows per call, rows per chunk, where the labels outside 0 .. 63 sit
  read(h, others, egos, ...)               the three outputs and the bad-label count of one call on tapped tokens h [B, A, 64]

The classes are the first maximum of numpy's float32 logits: the restatement is compared with its own variants only, never with
the device (the device's classes are held to the probes' own kernels and to float64 in test_gpu_bc_readout.py)."""
import numpy as np

f32 = np.float32
FILL = 255  # gd's GD_BC_READOUT_NO_CLASS: what a byte holds that no launch wrote

# (B, chunk_rows) -> the rows whose label is outside 0 .. 63, each where another part of the count decides it
TILE_CASES = {
    # the callers' default chunk: 4 ego tiles, two slots per lane in the bad-label count, a second chunk of 2.  Slot 0; a slot in
    # 64 .. 127 of the first chunk; a slot of an ego tile >= 1 below 64; the last slot of the first chunk; a slot of the second
    (130, 128): (0, 100, 40, 127, 129),
    # 3 ego tiles, the last with 6 live lanes; lanes 0 .. 5 take a second slot.  Slot 0; a second slot (lane 2); an ego tile
    # >= 1 below 64; the last slot
    (70, 70): (0, 66, 40, 69),
}
BAD_VALUES = (-1, 64, 1 << 40, -(1 << 40), 255)


def labels_with(B, bad_rows, seed=5):
    lab = np.random.default_rng(seed).integers(0, 64, B)
    for i, r in enumerate(bad_rows):
        lab[r] = BAD_VALUES[i % len(BAD_VALUES)]
    return lab


def list_case(B=130):
    """mask [B] bool with more than 64 listed rows, labels [B], the listed rows with a bad label, the unlisted ones.  Listed:
    the list's first row and a row at a list position >= 64; unlisted: a row of index >= 64."""
    rng = np.random.default_rng(17)
    mask = rng.random(B) < 0.75
    mask[[0, 1, B - 1]] = True, False, True
    listed = np.nonzero(mask)[0]
    assert len(listed) > 64
    late = int(listed[80])
    unlisted = int(np.nonzero(~mask)[0][-1])
    assert unlisted >= 64 and late >= 64
    lab = labels_with(B, (int(listed[0]), late, unlisted), seed=6)
    return mask, lab, (int(listed[0]), late), (unlisted,)


def probe_heads(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((64, 64)).astype(f32), rng.standard_normal(64).astype(f32)) for _ in range(n)]


def _classes(x, head):
    W, b = head
    return np.argmax(x.astype(f32) @ W.T + b, axis=-1).astype(np.uint8)  # (argmax: the first maximum)


def read(h, others, egos, labels=None, chunk_rows=128, rows=None, wrong=None):
    """h [B, A, 64] float32: token 0 the ego's, 1 + j partner column j's.  others / egos: lists of (weight [64, 64], bias [64]).
    labels: None, an int or [B].  rows: the listed rows in ascending order (None: every row).  Returns other_pred [B, n_other,
    A - 1], ego_pred [B, n_ego], ego_pred_prime [B, n_ego] (FILL where nothing is written) and the bad-label count.
    wrong:  'bad_first_64'  the count covers the slots below 64 of a chunk
            'prime_tile0'   the ego tiles from the second on write ego_pred and no prime
            'probe_cap3'    the probe index is capped at 3 (probes 4 .. 7 read probe 3's weights)
            'stride_A'      other_pred's column of probe q starts at q * A instead of q * (A - 1)"""
    B, A = h.shape[0], h.shape[1]
    n_other, n_ego = len(others), len(egos)
    os_ = n_other * (A - 1)
    other_pred = np.full(B * os_, FILL, np.uint8)  # flat: a store past a row's end lands in the next row, as on the device
    ego_pred, prime = np.full((B, n_ego), FILL, np.uint8), np.full((B, n_ego), FILL, np.uint8)
    bad = 0
    lab = None if labels is None else np.broadcast_to(np.asarray(labels, np.int64), (B,))
    index = (lambda q: min(q, 3)) if wrong == "probe_cap3" else (lambda q: q)
    positions = np.arange(B) if rows is None else np.asarray(rows)
    for r0 in range(0, B, chunk_rows):
        slots = min(chunk_rows, B - r0)
        sample = np.full(slots, -1)  # the row of a slot, -1 past the list
        live = positions[r0:r0 + slots]
        sample[:len(live)] = live
        tps = -(-(A - 1) // 32)
        for slot in range(slots if n_other else 0):  # partner tiles
            b = sample[slot]
            if b < 0:
                continue
            for i in range(tps):
                j = np.arange(32 * i, min(32 * i + 32, A - 1))
                for q in range(n_other):
                    at = b * os_ + q * (A if wrong == "stride_A" else A - 1) + j
                    c = _classes(h[b, 1 + j], others[index(q)])
                    other_pred[at[at < len(other_pred)]] = c[at < len(other_pred)]
        for tile in range(-(-slots // 32) if n_ego else 0):  # ego tiles
            b = sample[32 * tile:32 * tile + 32]
            b = b[b >= 0]
            if len(b) == 0 and tile != 0:
                continue
            for q in range(n_ego):
                ego_pred[b, q] = _classes(h[b, 0], egos[index(q)])
            if lab is None:
                continue
            ok = (lab[b] >= 0) & (lab[b] < 64)
            if not (wrong == "prime_tile0" and tile != 0):
                for p in range(n_ego):
                    w = others[index(p)][0][np.where(ok, lab[b], 0)]
                    x = np.where(ok[:, None], (h[b, 0] + w).astype(f32), h[b, 0])
                    prime[b, p] = _classes(x, egos[index(p)])
            if tile == 0:  # lane i takes the slots i, i + 64, ..
                for lane in range(64):
                    for s in range(lane, slots if wrong != "bad_first_64" else min(slots, 64), 64):
                        if sample[s] >= 0 and not 0 <= lab[sample[s]] < 64:
                            bad += 1
    out = {"ego_pred": ego_pred, "bad": bad}
    if n_other:
        out["other_pred"] = other_pred.reshape(B, n_other, A - 1)
    if lab is not None:
        out["ego_pred_prime"] = prime
    return out
