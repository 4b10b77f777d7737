"""Level-1 binning on the device (csrc/binning.hip: sb_count, sb_colscan, sb_scatter) at the shapes
where the scatter's rounds, mask words and footprint walks change path (level1_cases.py; the same
scenes whose index arithmetic test_level1_model_cpu.py rehearses on the CPU), in both binning
modes: the local sort runs the same kernel in its 16-byte-entry form over index order.

Each case first asserts, from the oracle's state, the facts that make it cover its path.  Integer
results (radii, keys, point list, ranges, and in global mode the depth order) are compared bit for
bit and everything else at the bars of test_gpu_parity.py, through that file's `compare`.  Chunks
longer than 1024 rows need more than 3.1M Gaussians: the 3M-row tests of test_gpu_parity.py and
the model's 2048-row case cover them.
"""
from __future__ import annotations

import numpy as np
import pytest

import level1_cases as L1
from test_gpu_parity import binning_mode, compare, run_hip, run_oracle, upstream_grads

_oracle = {}


def oracle_of(c):
    """Scene, oracle state and gradients of a case, computed once for both modes."""
    if c["name"] not in _oracle:
        s = L1.make_scene(c)
        dcol, dinv = upstream_grads(c)
        st, g = run_oracle(s, c, dcol, dinv)
        _oracle[c["name"]] = (s, dcol, dinv, st, g)
    return _oracle[c["name"]]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
@pytest.mark.parametrize("c", L1.CASES, ids=L1.IDS)
def test_level1_vs_oracle(c, mode):
    s, dcol, dinv, st, g = oracle_of(c)
    L1.check_facts(c, L1.facts(st))
    with binning_mode(mode):
        h = run_hip(s, c, dcol, dinv)
    compare(c, st, g, h, global_sort=mode == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
def test_same_frame_twice_same_lists(mode):
    """Ranks must not depend on timing: the same frame rendered twice gives the same raw
    (superblock-major) point list and ranges, bit for bit."""
    c = next(k for k in L1.CASES if k["name"] == "mixed_big_small")
    s = L1.make_scene(c)
    dcol, dinv = upstream_grads(c)
    with binning_mode(mode):
        a = run_hip(s, c, dcol, dinv)["state"]
        b = run_hip(s, c, dcol, dinv)["state"]
    assert len(a["point_list_raw"]) > 0
    np.testing.assert_array_equal(a["point_list_raw"], b["point_list_raw"])
    np.testing.assert_array_equal(a["ranges_raw"], b["ranges_raw"])
