"""Level-2 binning on the device (csrc/binning.hip: tile_bin, tb_split, and the local sort's
sb_sort_bin, all ranking through tb_rank) at the shapes where the walk changes path
(level2_cases.py; the same scenes whose arithmetic test_level2_model_cpu.py rehearses on the CPU):
list lengths around the waves' batch boundaries and around the LDS slots' capacity, an empty
superblock among full ones, partial superblocks, 8 x 8-tile superblocks, the 16-wave variant, a
list cut into slices, and equal depths -- in both binning modes and with the split gate off (the
splits armed on every frame) and on.

Each case first asserts, from the oracle's state, the facts that make it cover its path.  K, radii,
keys, point list and ranges are compared bit for bit and everything else at the bars of
test_gpu_parity.py, through that file's `compare`.  16 x 16-tile superblocks need a frame above
25 Mpix: the model alone covers them (test_model_shift4_crafted_lists, the shift-4 mask identity).
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import level1_cases as L1
import level2_cases as L2
from test_gpu_parity import binning_mode, compare, run_hip, run_oracle, upstream_grads

_oracle = {}


def oracle_of(c):
    """Scene, oracle state and gradients of a case, computed once for every mode and gate."""
    if c["name"] not in _oracle:
        s = L2.make_scene(c)
        dcol, dinv = upstream_grads(c)
        st, g = run_oracle(s, c, dcol, dinv)
        L2.check_facts(c, L2.facts(L1.preprocess_only(s, c), c["P"]))
        _oracle[c["name"]] = (s, dcol, dinv, st, g)
    return _oracle[c["name"]]


@contextlib.contextmanager
def split_gate(on):
    """gsr_set_split_gate for the duration: off arms the splits on every frame."""
    from diff_gaussian_rasterization import _C
    prev = _C.set_split_gate(bool(on))
    try:
        yield
    finally:
        _C.set_split_gate(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("gate", [0, 1], ids=["gate_off", "gate_on"])
@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
@pytest.mark.parametrize("c", L2.CASES, ids=L2.IDS)
def test_level2_vs_oracle(c, mode, gate):
    from diff_gaussian_rasterization import _C
    s, dcol, dinv, st, g = oracle_of(c)
    with binning_mode(mode), split_gate(gate):
        before = _C.forward_stats()["tb_split_frames"]
        h = run_hip(s, c, dcol, dinv)
        armed = _C.forward_stats()["tb_split_frames"] - before
    compare(c, st, g, h, global_sort=mode == 1)
    if c["name"] == "split_long_list" and mode == 1 and gate == 0:
        assert armed > 0, "the long list was not binned in slices"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
def test_same_frame_twice_same_lists(mode):
    """Ranks must not depend on timing: the same frame rendered twice gives the same raw
    (superblock-major) point list and ranges, bit for bit -- on a list walked in slot chunks."""
    c = L2.BY_NAME["corner_only"]
    s = L2.make_scene(c)
    dcol, dinv = upstream_grads(c)
    with binning_mode(mode):
        a = run_hip(s, c, dcol, dinv)["state"]
        b = run_hip(s, c, dcol, dinv)["state"]
    assert len(a["point_list_raw"]) > 0
    np.testing.assert_array_equal(a["point_list_raw"], b["point_list_raw"])
    np.testing.assert_array_equal(a["ranges_raw"], b["ranges_raw"])
