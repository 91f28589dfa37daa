"""Writes tests/golden/ref_domain.npz: the Peano-Hilbert key automaton that shq_peano_tables_from_key derives from the reference's
peano_hilbert_key, and the reference's PEANO() of the positions the key tests use (tests/domain_restated.py: key_positions).  The
tests read it where oracle/_ref has not been built; tests/test_domain_cpu.py holds it to the built library wherever both exist.

    make -C oracle ref && python tools/make_domain_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import domain_restated as dr  # noqa: E402

np.savez_compressed(dr.DOMAIN_GOLD, **dr.domain_store())
print("wrote", os.path.relpath(dr.DOMAIN_GOLD, ROOT), os.path.getsize(dr.DOMAIN_GOLD), "bytes")
