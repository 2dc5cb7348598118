"""sum_order.py, the numpy model of the fixed summation orders, against math.fsum: each order adds every term exactly once, so on
n terms it is within n 2^-53 sum |term| of the exact sum (n - 1 additions, each within 2^-53 of its own result <= sum |term|)."""
import math

import numpy as np
import pytest

import sum_order as SO

SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 1, 257 * 2048 + 3]


def mixed(n, seed):
    """n terms of both signs over twelve decades"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, n)


def check(got, terms):
    terms = np.asarray(terms, dtype=np.float64)
    bound = len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms))
    assert abs(float(got) - math.fsum(terms)) <= bound


@pytest.mark.parametrize("n", SIZES)
def test_two_level_sum(n):
    t = mixed(n, n)
    partials = SO.block_record_sum(t)
    assert partials.shape == ((n + 2047) // 2048,)
    for i in (0, len(partials) - 1) if n else ():
        check(partials[i], t[2048 * i:2048 * (i + 1)])
    check(SO.two_level_sum(partials), t)
    check(SO.fixed_sum(t), t)


def test_columns_are_summed_alike():
    t = np.stack([mixed(5000, 1), mixed(5000, 2), mixed(5000, 3)], axis=1)
    got = SO.fixed_sum(t)
    assert got.shape == (3,)
    for k in range(3):
        assert got[k] == SO.fixed_sum(t[:, k])
    seg = SO.segment_sum(t, 17, 4000)
    for k in range(3):
        assert seg[k] == SO.segment_sum(t[:, k], 17, 4000)


def test_order_is_the_documented_one():
    """small enough to write out: 2 ** 53 absorbs a 1.0 added to it, so the result tells the order"""
    big = 2.0 ** 53
    t = np.zeros(2048)
    t[0], t[256], t[32] = big, 1.0, 1.0  # thread 0 adds items 0 and 256: big + 1 = big; lane 32 brings the other 1: big again
    assert SO.block_record_sum(t)[0] == big
    t = np.zeros(2048)
    t[0], t[32], t[288] = big, 1.0, 1.0  # thread 32 adds items 32 and 288: 2, and big + 2 is exact
    assert SO.block_record_sum(t)[0] == big + 2.0
    p = np.zeros(513)
    p[0], p[256], p[512] = big, 1.0, 1.0  # the final kernel's thread 0 adds records 0, 256, 512 in turn
    assert SO.two_level_sum(p) == big
    s = np.zeros(130)
    s[0], s[1], s[65] = big, 1.0, 1.0  # a long segment: lane 1 adds items 1 and 65, in order they would both be lost
    assert SO.segment_sum(s, 0, 130) == big + 2.0
    s = np.zeros(64)
    s[0], s[1], s[33] = big, 1.0, 1.0  # a short one goes in order, not through the tree
    assert SO.segment_sum(s, 0, 64) == big


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 129, 300, 4097])
def test_segment_sum(length):
    t = mixed(length + 200, length)
    check(SO.segment_sum(t, 100, 100 + length), t[100:100 + length])


@pytest.mark.parametrize("b,e", [(100, 100 + 2 * 2048 + 300), (4861, 4861 + 3 * 2048 + 300), (4561, 4861), (0, 2048), (2048, 6144),
                                 (2047, 4097)])
def test_segment_sum_through_block_sums(b, e):
    t = mixed(12000, b)
    sums = SO.block_record_sum(t)
    check(SO.segment_sum(t, b, e, sums), t[b:e])
    if -(-b // 2048) >= e // 2048:
        assert SO.segment_sum(t, b, e, sums) == SO.segment_sum(t, b, e)
