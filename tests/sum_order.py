"""The three fixed summation orders of csrc/fixed_sums.h as plain float64 numpy ("Fixed-order sums").  IEEE double
addition without contraction leaves no freedom, so a device sum must equal its model bit for bit (test_hip_fixed_sums.py);
test_sum_order_cpu.py holds the models themselves against math.fsum.

Terms are (n,) or (n, K): K sums side by side, each in the same order.  An item that a lane skips is a +0.0 at its place: an
accumulator starts at +0.0 and +0.0 + x, x + +0.0 leave x's bits for every x a sum of these can reach (no accumulator is ever -0.0).
"""
import numpy as np

WAVE = 64


def _columns(terms):
    a = np.asarray(terms, dtype=np.float64)
    return a.reshape(len(a), int(np.prod(a.shape[1:]))), a.shape[1:]


def _in_turn(a):
    """(steps, ...) -> the running sum from +0.0 over axis 0, one step after the other"""
    acc = np.zeros(a.shape[1:])
    for row in a:
        acc = acc + row
    return acc


def wave_tree(v):
    """(..., 64, K) -> (..., K): v += shfl_xor(v, s) for s = 32 .. 1 as lane 0 sees it (every lane holds the same bits: a + b = b + a)"""
    for s in (32, 16, 8, 4, 2, 1):
        v = v[..., :s, :] + v[..., s:2 * s, :]
    return v[..., 0, :]


def workgroup_sum(acc):
    """(B, threads, K) per-thread values -> (B, K): the tree inside each wave, then the waves added in wave order"""
    B, threads, K = acc.shape
    w = wave_tree(acc.reshape(B, threads // WAVE, WAVE, K))
    out = w[:, 0]
    for i in range(1, threads // WAVE):
        out = out + w[:, i]
    return out


def _strided(a, lanes):
    """(n, K) -> (lanes, K): lane l adds items l, l + lanes, ... in that order"""
    steps = -(-len(a) // lanes)
    pad = np.zeros((steps * lanes, a.shape[1]))
    pad[:len(a)] = a
    return _in_turn(pad.reshape(steps, lanes, a.shape[1]))


def block_record_sum(terms, threads=256, per_thread=8):
    """One record per workgroup of threads * per_thread consecutive items -> (blocks, ...): thread i of a block adds its items
    base + i + k * threads for k ascending, then workgroup_sum."""
    a, tail = _columns(terms)
    per = threads * per_thread
    blocks = -(-len(a) // per)
    pad = np.zeros((blocks * per, a.shape[1]))
    pad[:len(a)] = a
    acc = _in_turn(pad.reshape(blocks, per_thread, threads, a.shape[1]).transpose(1, 0, 2, 3))
    return workgroup_sum(acc).reshape((blocks,) + tail)


def two_level_sum(partials, threads=256):
    """The final kernel over the blocks' records -> (...): thread t adds records t, t + threads, ..., then workgroup_sum."""
    a, tail = _columns(partials)
    return workgroup_sum(_strided(a, threads)[None])[0].reshape(tail)


def fixed_sum(terms, threads=256, per_thread=8):
    """block_record_sum, then two_level_sum: what mvd_cloud_scores_f32 and mvd_cloud_pair_sums_f32 return for their terms"""
    return two_level_sum(block_record_sum(terms, threads, per_thread), threads)


def _span(a):
    return _strided(a, WAVE)


def segment_sum(terms, b, e, block_sums=None, block=2048):
    """The sum of terms[b:e] as the segment walk forms it -> (...).  At most 64 items: one after the other.  More: lane l adds
    items l, l + 64, ... of the segment and the wave tree joins the lanes.  With block_sums (the mesh variant; block_sums[i] =
    block_record_sum(terms)[i]) a long segment that holds whole blocks of `block` positions is, per lane, its head up to the first
    block boundary, then the stored sums of its whole blocks, then its tail."""
    a, tail = _columns(terms)
    if e - b <= WAVE:
        return _in_turn(a[b:e]).reshape(tail)
    first, last = -(-b // block), e // block
    if block_sums is None or first >= last:
        lanes = _span(a[b:e])
    else:
        sums = np.asarray(block_sums, dtype=np.float64).reshape(-1, a.shape[1])
        lanes = (_span(a[b:first * block]) + _span(sums[first:last])) + _span(a[last * block:e])
    return wave_tree(lanes).reshape(tail)
