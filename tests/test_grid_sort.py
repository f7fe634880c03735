"""Grider_GRID.h:128's std::sort of a cell's FAST keypoints (CPU; VERDICT r05 missing #1).

The reference sorts each cell's cv::FAST output (raster order) with std::sort and the response-only
Grider_FAST::compare_response (Grider_FAST.h:57).  std::sort is libstdc++'s introsort, which is not stable:
the tie order of equal responses decides which corners a cell keeps and the order they get their ids
(TrackKLT.cpp:483-520).  Three statements of it are checked against each other here:

  * the oracle (oracle/src/tracker.cpp grid_sort): libstdc++'s own std::sort, called on the cv::FAST sequence;
  * `_libstdcxx_sort`: a literal Python restatement of libstdc++'s stl_algo.h / stl_heap.h (introsort loop
    with _S_threshold 16, __move_median_to_first, __unguarded_partition, the __partial_sort heap fallback at
    depth 2 lg n, __final_insertion_sort) -- pins that the oracle runs that algorithm (the same code in the
    GCC 7-13 libstdc++ of the ROS distributions the reference builds on);
  * `_device_model`: the formulation the device kernel runs (kernels_track.hip grid_introsort): every
    partition step from ballot ranks of the scans' stop positions, the sorted order as the stable order of
    the introsort loop's arrangement, segments below the k-th largest response left unrefined.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _lg(n):
    return n.bit_length() - 1


def _heap_adjust(a, first, hole, length, value, gt):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if gt(a[first + second], a[first + second - 1]):
            second -= 1
        a[first + hole] = a[first + second]
        hole = second
    if (length & 1) == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        a[first + hole] = a[first + second - 1]
        hole = second - 1
    parent = (hole - 1) // 2
    while hole > top and gt(a[first + parent], value):
        a[first + hole] = a[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[first + hole] = value


def _partial_sort_all(a, first, last, gt):
    n = last - first
    if n >= 2:
        parent = (n - 2) // 2
        while True:
            _heap_adjust(a, first, parent, n, a[first + parent], gt)
            if parent == 0:
                break
            parent -= 1
    while last - first > 1:
        last -= 1
        v = a[last]
        a[last] = a[first]
        _heap_adjust(a, first, 0, last - first, v, gt)


def _libstdcxx_sort(resp, depth_limit=None):
    """std::sort(v.begin(), v.end(), [](a, b) { return a.response > b.response; }) over (response, raster idx),
    statement by statement after libstdc++'s stl_algo.h; returns the raster indices in sorted order."""
    a = [(float(r), i) for i, r in enumerate(resp)]
    gt = lambda x, y: x[0] > y[0]  # noqa: E731
    n = len(a)

    def introsort_loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                _partial_sort_all(a, first, last, gt)
                return
            depth -= 1
            mid = first + (last - first) // 2
            x, y, z = first + 1, mid, last - 1
            if gt(a[x], a[y]):
                m = y if gt(a[y], a[z]) else (z if gt(a[x], a[z]) else x)
            elif gt(a[x], a[z]):
                m = x
            elif gt(a[y], a[z]):
                m = z
            else:
                m = y
            a[first], a[m] = a[m], a[first]
            lo, hi = first + 1, last
            while True:
                while gt(a[lo], a[first]):
                    lo += 1
                hi -= 1
                while gt(a[first], a[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                a[lo], a[hi] = a[hi], a[lo]
                lo += 1
            introsort_loop(lo, last, depth)
            last = lo

    def linear_insert(i):
        v = a[i]
        j = i - 1
        while gt(v, a[j]):
            a[j + 1] = a[j]
            j -= 1
        a[j + 1] = v

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if gt(a[i], a[first]):
                v = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = v
            else:
                linear_insert(i)

    if n:
        introsort_loop(0, n, 2 * _lg(n) if depth_limit is None else depth_limit)
        if n > 16:
            insertion_sort(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion_sort(0, n)
    return [i for _, i in a]


def _device_model(resp, t=-1, depth=None):
    """kernels_track.hip grid_introsort: the introsort loop's arrangement computed partition by partition from
    the ranks of the scans' stop positions (L_k: response <= pivot from the left, R_k: >= pivot from the
    right; swap k iff L_k < R_k; cut = min(L_{K+1}, R_K)); segments whose responses are all below t skipped."""
    n = len(resp)
    a = [(int(r), i) for i, r in enumerate(resp)]
    if n > 16:
        stk = [(0, n, 2 * _lg(n) if depth is None else depth, 255)]
        while stk:
            f, l, d, ub = stk.pop()
            while l - f > 16 and ub >= t:
                if d == 0:
                    _partial_sort_all(a, f, l, lambda x, y: x[0] > y[0])
                    break
                d -= 1
                mid = f + (l - f) // 2
                ra, rb, rc = a[f + 1][0], a[mid][0], a[l - 1][0]
                if ra > rb:
                    m = mid if rb > rc else (l - 1 if ra > rc else f + 1)
                elif ra > rc:
                    m = f + 1
                elif rb > rc:
                    m = l - 1
                else:
                    m = mid
                a[f], a[m] = a[m], a[f]
                p = a[f][0]
                pl = [i for i in range(f + 1, l) if a[i][0] <= p]
                pr = [i for i in range(f + 1, l) if a[i][0] >= p]
                K = 0
                while K < min(len(pl), len(pr)) and pl[K] < pr[len(pr) - 1 - K]:
                    K += 1
                cut = min(pl[K] if K < len(pl) else l, pr[len(pr) - K] if K > 0 else l)
                for k in range(K):
                    x, y = pl[k], pr[len(pr) - 1 - k]
                    a[x], a[y] = a[y], a[x]
                if l - cut > 16 and p >= t:
                    stk.append((cut, l, d, p))
                l = cut
    return [i for _, i in sorted(a, key=lambda v: -v[0])]  # the final insertion sort: stable over the arrangement


def _cells(rng, count, nmax=400):
    out = []
    for _ in range(count):
        n = int(rng.integers(1, nmax))
        spread = int(rng.choice([2, 5, 12, 40, 200]))
        out.append(rng.integers(21, 21 + spread, n).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_oracle_is_libstdcxx_std_sort(O):
    rng = np.random.default_rng(11)
    for r in _cells(rng, 600):
        assert list(O.grid_order(r, 0)) == _libstdcxx_sort(r)
    # the heap-sort fallback (std::partial_sort over the whole range) of the same restatement
    # (above 16 elements: std::sort leaves at most 16 to the insertion sort alone)
    for r in _cells(rng, 150):
        if len(r) > 16:
            assert list(O.grid_order(r, 2)) == _libstdcxx_sort(r, depth_limit=0)


def test_device_formulation_equals_std_sort(O):
    rng = np.random.default_rng(12)
    for r in _cells(rng, 800):
        ref = list(O.grid_order(r, 0))
        assert _device_model(r) == ref
        k = int(rng.integers(1, 65))
        m = min(k, len(r))
        t = np.sort(r)[::-1][m - 1]
        assert _device_model(r, t=t)[:m] == ref[:m]  # pruned below the cell's m-th response
        if len(r) > 16:
            assert _device_model(r, depth=0) == list(O.grid_order(r, 2))


def test_std_sort_order_is_not_the_stable_order(O):
    """The verdict's count: top-17 of 17-96 tied integer responses differ from the stable order in most cells;
    at most 16 candidates (insertion sort only) the two agree."""
    rng = np.random.default_rng(13)
    differ = 0
    for _ in range(1000):
        n = int(rng.integers(17, 97))
        r = rng.integers(21, 41, n).astype(np.float32)
        differ += list(O.grid_order(r, 0)[:17]) != list(O.grid_order(r, 1)[:17])
    assert differ > 900, differ
    for _ in range(300):
        r = rng.integers(21, 25, int(rng.integers(1, 17))).astype(np.float32)
        assert list(O.grid_order(r, 0)) == list(O.grid_order(r, 1))


def test_griding_keeps_std_sort_top_k(O):
    """perform_griding's per-cell pick on a corner-dense image equals FAST (raster order) + std::sort, and differs
    from the stable pick on some cells (so the tracker tests see the difference)."""
    rng = np.random.default_rng(3)
    img = (rng.integers(0, 2, (96, 160)) * 200 + 20).astype(np.uint8)
    img = np.kron(img, np.ones((2, 2), dtype=np.uint8))[:192, :320].copy()
    nfg = 9
    differ = 0
    for cy in range(0, 192, 64):
        for cx in range(0, 320, 64):
            kp = O.fast(img, 20, roi=(cx, cy, 64, 64))
            order = O.grid_order(kp[:, 2], 0)
            stable = O.grid_order(kp[:, 2], 1)
            assert len(kp) > 16
            differ += list(order[:nfg]) != list(stable[:nfg])
    assert differ > 0


def test_probe_refuses_depth_beyond_its_stack():
    """uvio_hp_debug_grid_order with a depth limit above the kernel's 64-entry segment stack is UVIO_HP_E_ARG, found
    in the argument checks: no device is needed to be told so (without one an accepted depth gets as far as
    UVIO_HP_E_DEVICE)."""
    from uvio_amd.manager import grid_order
    cell = [np.array([30, 25, 30, 22])]
    with pytest.raises(RuntimeError, match="E_ARG"):
        grid_order(cell, kmax=0, depth=65)
