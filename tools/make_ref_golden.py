"""Store under tests/golden/ what the reference-built pieces of oracle/_ref give for the inputs the tests use, so that those tests run
where the reference's sources are absent and oracle/_ref cannot be built (tests/ref_outputs.py serves them).  Needs oracle/_ref
(`make -C oracle ref`):
    python tools/make_ref_golden.py
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_outputs as ro  # noqa: E402

lib = ro.peano_lib()
for path in (ro.PEANO_LIB, ro.LAYOUT_PROBE, ro.DENSITYKERNEL_LIB, ro.SHORTRANGE_LIB):
    if not os.path.exists(path):
        raise SystemExit("%s missing: run `make -C oracle ref` first" % os.path.relpath(path, ROOT))

# Peano-Hilbert keys: the small hilbert_key tables, the full keys the tests compare, the top leaves of the top-leaf cases
store = ro.peano_store(ro.Peano(lib=lib))
np.savez_compressed(ro.PEANO_GOLD, **store)

# struct layouts: the probe's output as it prints it
with open(ro.LAYOUT_GOLD, "w") as f:
    f.write(subprocess.check_output([ro.LAYOUT_PROBE]).decode())

# SPH kernels on the seeded arguments of test_density_kernel_vs_reference_build
np.savez_compressed(ro.DENSITYKERNEL_GOLD, args=np.array(ro.densitykernel_args()), out=ro.densitykernel_outputs(ro.densitykernel_lib()))

# the tabulated short-range window: its digest (the table itself ships as shenqi_amd/data/shortrange_force_kernels.f64)
with open(ro.SHORTRANGE_GOLD, "w") as f:
    json.dump(ro.table_digest(ro.shortrange_table_lib()), f)
    f.write("\n")
print("stored %d Peano keys and %d top leaves, the layout probe's output, %d kernel evaluations and the window table's digest under "
      "tests/golden/" % (len(store["key"]), sum(len(v) for k, v in store.items() if k.startswith("leaf_")), len(ro.densitykernel_args())))
