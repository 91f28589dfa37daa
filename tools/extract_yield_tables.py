"""Write tests/golden/metal_yield_tables.npz: the numbers of the reference's libgadget/metal_tables.h as arrays (data only).

    python tools/extract_yield_tables.py <path to metal_tables.h> [out.npz]

The header is read as text: the `#define NAME number` lines and the brace-enclosed initialisers of the `static const double` arrays.
Tables keep the header's layout: value[mass index * nmet + metallicity index]; the species tables are [NSPECIES][nmass * nmet]."""
import os
import re
import sys

import numpy as np

NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defs = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define\s+(\w+)\s+(" + NUM + r")\s*$", text, flags=re.M)}
    arrays = {}
    for m in re.finditer(r"static\s+const\s+double\s+(\w+)\s*((?:\[[^\]]*\])*)\s*=\s*([^;]*);", text, flags=re.S):
        arrays[m.group(1)] = np.array([float(x) for x in re.findall(NUM, m.group(3))])
    return defs, arrays


def main():
    src = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "metal_yield_tables.npz")
    with open(src) as f:
        defs, a = parse(f.read())
    ns = int(defs["NSPECIES"])
    dims = {k: int(defs[k]) for k in ("LIFE_NMET", "LIFE_NMASS", "AGB_NMET", "AGB_NMASS", "SNII_NMET", "SNII_NMASS")}
    assert a["lifetime"].size == dims["LIFE_NMET"] * dims["LIFE_NMASS"] and a["lifetime_masses"].size == dims["LIFE_NMASS"]
    assert a["agb_total_mass"].size == a["agb_total_metals"].size == dims["AGB_NMET"] * dims["AGB_NMASS"]
    assert a["agb_yield"].size == ns * dims["AGB_NMET"] * dims["AGB_NMASS"]
    assert a["snii_total_mass"].size == a["snii_total_metals"].size == dims["SNII_NMET"] * dims["SNII_NMASS"]
    assert a["snii_yield"].size == ns * dims["SNII_NMET"] * dims["SNII_NMASS"] and a["sn1a_yields"].size == ns
    np.savez(out, MAXMASS=defs["MAXMASS"], MINMASS=defs["MINMASS"], SNAGBSWITCH=defs["SNAGBSWITCH"],
             lifetime_metallicity=a["lifetime_metallicity"], lifetime_masses=a["lifetime_masses"], lifetime=a["lifetime"],
             agb_masses=a["agb_masses"], agb_metallicities=a["agb_metallicities"], agb_total_mass=a["agb_total_mass"],
             agb_total_metals=a["agb_total_metals"], agb_yield=a["agb_yield"].reshape(ns, -1),
             snii_masses=a["snii_masses"], snii_metallicities=a["snii_metallicities"], snii_total_mass=a["snii_total_mass"],
             snii_total_metals=a["snii_total_metals"], snii_yield=a["snii_yield"].reshape(ns, -1),
             sn1a_total_metals=a["sn1a_total_metals"][0], sn1a_yields=a["sn1a_yields"])
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
