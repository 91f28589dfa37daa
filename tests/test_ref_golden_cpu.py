"""The outputs of the reference-built pieces stored under tests/golden/ (tools/make_ref_golden.py) against those pieces, where
oracle/_ref has been built: the stored values the tests fall back on are the ones the reference gives."""
import json
import os

import numpy as np
import pytest

import ref_outputs as ro


@pytest.mark.skipif(not os.path.exists(ro.PEANO_LIB), reason="oracle/_ref not built")
def test_stored_peano_keys_are_the_reference_s():
    want = ro.peano_store(ro.Peano(lib=ro.peano_lib()))
    g = np.load(ro.PEANO_GOLD)
    assert sorted(g.files) == sorted(want)
    for name in want:
        assert np.array_equal(g[name], want[name]), name


@pytest.mark.skipif(not os.path.exists(ro.LAYOUT_PROBE), reason="oracle/_ref not built")
def test_stored_layout_is_the_probe_s():
    assert json.load(open(ro.LAYOUT_GOLD)) == ro.layout()


@pytest.mark.skipif(not os.path.exists(ro.DENSITYKERNEL_LIB), reason="oracle/_ref not built")
def test_stored_density_kernels_are_the_reference_s():
    g = np.load(ro.DENSITYKERNEL_GOLD)
    assert np.array_equal(g["args"], np.array(ro.densitykernel_args()))
    assert np.array_equal(g["out"], ro.densitykernel_outputs(ro.densitykernel_lib()))


@pytest.mark.skipif(not os.path.exists(ro.SHORTRANGE_LIB), reason="oracle/_ref not built")
def test_stored_window_digest_is_the_reference_table_s():
    assert json.load(open(ro.SHORTRANGE_GOLD)) == ro.table_digest(ro.shortrange_table_lib())
