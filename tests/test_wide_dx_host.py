"""CPU: the entry points of csrc/dense_dx_split_bf16.hip refuse bad arguments on the host, before anything is enqueued, and the
predicate that hands the wide input gradient to them (dense.wide_dx_takes) says no without a device."""
import pytest
import torch

from geometrics_amd import _lib, dense

EINVAL, EUNSUPPORTED = -1, _lib.EUNSUPPORTED


def test_entry_points_validate_before_any_launch():
    L = _lib.lib()
    assert [L.geom_dense_dx_split_cinpad(n) for n in (0, 1, 32, 33, 963, 1155)] == [0, 32, 32, 64, 992, 1184]
    a = 4096                                               # an aligned non-null address nobody dereferences on the host
    assert L.geom_dense_dx_split_planes_f32(0, 192, a, a, None) == EINVAL
    assert L.geom_dense_dx_split_planes_f32(963, 96, a, a, None) == EUNSUPPORTED
    assert L.geom_dense_dx_split_planes_f32(963, 192, None, a, None) == EINVAL
    assert L.geom_dense_dx_split_planes_f32(963, 192, a, a + 8, None) == EINVAL
    assert L.geom_dense_dx_split_f32(-1, 963, 192, a, a, a, 963, None) == EINVAL
    assert L.geom_dense_dx_split_f32(5, 963, 96, a, a, a, 963, None) == EUNSUPPORTED
    assert L.geom_dense_dx_split_f32(5, 963, 192, a, a, a, 962, None) == EINVAL           # pitch below the row length
    assert L.geom_dense_dx_split_f32(5, 963, 192, a + 4, a, a, 963, None) == EINVAL       # g not 16-byte aligned
    assert L.geom_dense_dx_split_f32(5, 963, 192, a, None, a, 963, None) == EINVAL
    assert L.geom_dense_dx_split_f32(0, 963, 192, None, None, None, 963, None) == 0       # no rows: nothing to do


def test_the_predicate_and_the_plan(monkeypatch):
    monkeypatch.delenv("GEOM_WIDE_DX", raising=False)
    assert dense.wide_dx_plan(20496, 963, 192) and not dense.wide_dx_plan(648, 963, 192)
    assert not dense.wide_dx_plan(20496, 192, 192) and not dense.wide_dx_plan(20496, 963, 96)
    assert not dense.wide_dx_plan(7712, 1155, 192)        # the driver step's shape: level with the library, left with it
    g, w = torch.zeros(20496, 192), torch.zeros(963, 192)
    for mode in (None, "split", "lib"):
        monkeypatch.setattr(dense, "wide_dx", mode)
        assert not dense.wide_dx_takes(g, w)               # host tensors: never
    monkeypatch.setattr(dense, "wide_dx", "fast")
    with pytest.raises(ValueError):
        dense.wide_dx_takes(g, w)
