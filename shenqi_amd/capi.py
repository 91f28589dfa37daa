"""ctypes bindings of the C-ABI (include/shenqi_hip.h) and of the host mirror library.

The compute lives in shenqi_amd/lib/libshenqi_hip.so (hand-written HIP for gfx950).  There is
no Python or CPU fallback: if the library is missing, importing this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.environ.get("SHQ_LIBDIR") or os.path.join(_HERE, "lib")   # SHQ_LIBDIR: an alternative build of the two libraries (tuning experiments)
DATADIR = os.path.join(_HERE, "data")

NGRAVTAB = 512
NMAXCHILD = 8
NOFIELD = C.c_size_t(-1).value

WALK_EXACT = 0
WALK_GROUP = 1
WALK_AUTO = 2
WALK_TREE_ORDER = 0x100
WALK_DEFER_POSTPROCESS = 0x200


class ShqError(RuntimeError):
    """Non-zero status from the library (the shim's endrun() equivalent)."""


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). shenqi_amd has no fallback path."
        )
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


hip = _load("libshenqi_hip.so")
host = _load("libshenqi_host.so")


# ---- POD mirrors ---------------------------------------------------------------------------
class PartView(C.Structure):
    _fields_ = [
        ("base", C.c_void_p), ("elsize", C.c_size_t), ("numpart", C.c_int64),
        ("off_pos", C.c_size_t), ("off_mass", C.c_size_t), ("off_type", C.c_size_t),
        ("off_flags", C.c_size_t), ("off_pi", C.c_size_t), ("off_vel", C.c_size_t),
        ("off_treeacc", C.c_size_t), ("off_gravpm", C.c_size_t), ("off_potential", C.c_size_t),
        ("off_hsml", C.c_size_t), ("off_dthsml", C.c_size_t),
        ("off_timebin_hydro", C.c_size_t), ("off_timebin_gravity", C.c_size_t),
    ]


class Node(C.Structure):
    _fields_ = [
        ("sibling", C.c_int32), ("father", C.c_int32), ("len", C.c_double),
        ("center", C.c_double * 3), ("cofm", C.c_double * 3), ("mass", C.c_double),
        ("hmax", C.c_double), ("suns", C.c_int32 * NMAXCHILD), ("noccupied", C.c_int32),
        ("flags", C.c_uint32),
    ]


NODE_DTYPE = np.dtype(
    {
        "names": ["sibling", "father", "len", "center", "cofm", "mass", "hmax", "suns", "noccupied", "flags"],
        "formats": ["<i4", "<i4", "<f8", ("<f8", 3), ("<f8", 3), "<f8", "<f8", ("<i4", 8), "<i4", "<u4"],
        "offsets": [0, 4, 8, 16, 40, 64, 72, 80, 112, 116],
        "itemsize": 120,
    }
)
assert C.sizeof(Node) == 120

# struct particle_data, libgadget/partmanager.h:9-71 (160 B)
PARTICLE_DTYPE = np.dtype(
    {
        "names": ["Pos", "TopLeaf", "Mass", "PI", "Flags", "TimeBinHydro", "TimeBinGravity", "Type", "Vel",
                  "FullTreeGravAccel", "GravPM", "Ti_drift", "Hsml", "DtHsml", "ID", "GrNr", "Potential"],
        "formats": [("<f8", 3), "<i4", "<f4", "<i4", "u1", "u1", "u1", "u1", ("<f8", 3), ("<f8", 3), ("<f8", 3),
                    "<i8", "<f8", "<f8", "<u8", "<i8", "<f8"],
        "offsets": [0, 24, 28, 32, 36, 37, 38, 39, 40, 64, 88, 112, 120, 128, 136, 144, 152],
        "itemsize": 160,
    }
)

# struct sph_particle_data, libgadget/slotsmanager.h:97-131 (176 B)
SPH_DTYPE = np.dtype(
    {
        "names": ["ReverseLink", "Density", "EgyWtDensity", "Entropy", "DtEntropy", "MaxSignalVel", "HydroAccel",
                  "DhsmlEgyDensityFactor", "DivVel", "CurlVel", "Sfr", "Ne", "VDisp", "DelayTime", "Metallicity", "Metals"],
        "formats": ["<i4", "<f8", "<f8", "<f8", "<f8", "<f8", ("<f8", 3), "<f8", "<f8", "<f8", "<f8", "<f8", "<f8",
                    "<f8", "<f8", ("<f4", 9)],
        "offsets": [0, 8, 16, 24, 32, 40, 48, 72, 80, 88, 96, 104, 112, 120, 128, 136],
        "itemsize": 176,
    }
)


class TreeView(C.Structure):
    _fields_ = [
        ("nodes_base", C.c_void_p), ("firstnode", C.c_int64), ("lastnode", C.c_int64),
        ("numnodes", C.c_int64), ("rootnode", C.c_int32), ("full_particle_tree_flag", C.c_int32),
        ("BoxSize", C.c_double), ("father", C.c_void_p),
    ]


class GravParams(C.Structure):
    _fields_ = [
        ("BoxSize", C.c_double), ("cellsize", C.c_double), ("Rcut", C.c_double), ("G", C.c_double),
        ("cbrtrho0", C.c_double), ("ForceSoftening", C.c_double), ("ErrTolForceAcc", C.c_double),
        ("BHOpeningAngle2", C.c_double), ("TreeUseBH", C.c_int32), ("pad_", C.c_int32),
        ("shortrange_table", C.c_float * NGRAVTAB), ("shortrange_table_potential", C.c_float * NGRAVTAB),
        ("dx", C.c_double),
    ]


class TreeBuildStats(C.Structure):
    _fields_ = [("nparticles", C.c_int64), ("numnodes", C.c_int64), ("maxdepth", C.c_int32), ("build_ms", C.c_float)]


TIMEBINS = 46


class ActiveInfo(C.Structure):
    _fields_ = [("NumActiveParticle", C.c_int64), ("NumActiveGravity", C.c_int64), ("NumActiveHydro", C.c_int64),
                ("TimeBinCountType", C.c_int64 * (6 * (TIMEBINS + 1)))]


ACTIVE_RESIDENT = C.c_void_p(2**64 - 1)    # SHQ_ACTIVE_RESIDENT
SUBLIST_RESIDENT = C.c_void_p(2**64 - 2)   # SHQ_SUBLIST_RESIDENT


class WalkStats(C.Structure):
    _fields_ = [
        ("ntargets", C.c_int64), ("ninteractions", C.c_int64), ("min_interactions", C.c_int64),
        ("max_interactions", C.c_int64), ("nnodes_visited", C.c_int64), ("nwave_interactions", C.c_int64),
        ("nwave_node_interactions", C.c_int64), ("nnode_interactions", C.c_int64),
        ("kernel_ms", C.c_double),
    ]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}




class KickFactors(C.Structure):
    _fields_ = [("FgravkickB", C.c_double), ("gravkicks", C.c_double * (TIMEBINS + 1)),
                ("hydrokicks", C.c_double * (TIMEBINS + 1)), ("dloga_kick", C.c_double * (TIMEBINS + 1)),
                ("dloga_for_bin", C.c_double * (TIMEBINS + 1))]


class DensityParams(C.Structure):
    _fields_ = [("BoxSize", C.c_double), ("DesNumNgb", C.c_double), ("DesNumNgbBH", C.c_double),
                ("MinGasHsml", C.c_double), ("MaxNumNgbDeviation", C.c_double), ("update_hsml", C.c_int32),
                ("BlackHoleOn", C.c_int32), ("DoEgyDensity", C.c_int32), ("WindsDecouple", C.c_int32),
                ("DensityKernelType", C.c_int32), ("pad_", C.c_int32), ("kf", KickFactors)]


class HydroParams(C.Structure):
    _fields_ = [("BoxSize", C.c_double), ("atime", C.c_double), ("fac_mu", C.c_double), ("fac_vsic_fix", C.c_double),
                ("hubble_a2", C.c_double), ("drifts", C.c_double * (TIMEBINS + 1)), ("ArtBulkViscConst", C.c_double),
                ("DensityContrastLimit", C.c_double), ("WindSpeed", C.c_double), ("WindFreeTravelDensThresh", C.c_double),
                ("DensityIndependentSphOn", C.c_int32), ("DensityKernelType", C.c_int32), ("kf", KickFactors)]


class SphView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64),
                ("off_density", C.c_size_t), ("off_egywtdensity", C.c_size_t), ("off_entropy", C.c_size_t),
                ("off_dtentropy", C.c_size_t), ("off_maxsignalvel", C.c_size_t), ("off_hydroaccel", C.c_size_t),
                ("off_dhsmlegydensityfactor", C.c_size_t), ("off_divvel", C.c_size_t), ("off_curlvel", C.c_size_t),
                ("off_delaytime", C.c_size_t)]


# struct bh_particle_data, libgadget/slotsmanager.h:35-73 (248 B)
BH_DTYPE = np.dtype(
    {
        "names": ["ReverseLink", "minTimeBin", "encounter", "TimeBinDynFric", "JumpToMinPot", "Mass", "Mdot", "Density", "DivVel", "Mtrack",
                  "KineticFdbkEnergy", "VDisp", "DFAccel", "DF_SurroundingVel", "DF_SurroundingRmsVel", "DF_SurroundingDensity", "DragAccel",
                  "SwallowTime", "SwallowID", "Mseed", "FormationTime", "MinPot", "MinPotPos", "MinPotVel", "CountProgs"],
        "formats": ["<i4", "u1", "i1", "u1", "i1", "<f8", "<f8", "<f8", "<f8", "<f8", "<f8", "<f8", ("<f8", 3), ("<f8", 3), "<f8", "<f8",
                    ("<f8", 3), "<f8", "<u8", "<f8", "<f8", "<f8", ("<f8", 3), ("<f8", 3), "<i4"],
        "offsets": [0, 4, 5, 6, 7, 8, 16, 24, 32, 40, 48, 56, 64, 88, 112, 120, 128, 152, 160, 168, 176, 184, 192, 216, 240],
        "itemsize": 248,
    }
)


class BhDynView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64),
                ("off_mintimebin", C.c_size_t), ("off_timebindynfric", C.c_size_t), ("off_jumptominpot", C.c_size_t),
                ("off_dfaccel", C.c_size_t), ("off_df_surroundingvel", C.c_size_t), ("off_dragaccel", C.c_size_t),
                ("off_minpotpos", C.c_size_t), ("off_minpotvel", C.c_size_t)]


def bh_dyn_view(BhP):
    """shq_bh_dyn_view of a numpy array of BH_DTYPE records."""
    v = BhDynView()
    f = BhP.dtype.fields
    v.base, v.elsize, v.numslots = BhP.ctypes.data, BhP.dtype.itemsize, len(BhP)
    v.off_mintimebin, v.off_timebindynfric, v.off_jumptominpot = f["minTimeBin"][1], f["TimeBinDynFric"][1], f["JumpToMinPot"][1]
    v.off_dfaccel, v.off_df_surroundingvel, v.off_dragaccel = f["DFAccel"][1], f["DF_SurroundingVel"][1], f["DragAccel"][1]
    v.off_minpotpos, v.off_minpotvel = f["MinPotPos"][1], f["MinPotVel"][1]
    return v


class ExchangeLayout(C.Structure):
    _fields_ = [("part_elsize", C.c_size_t), ("off_flags", C.c_size_t), ("off_type", C.c_size_t), ("off_pi", C.c_size_t),
                ("slot_elsize", C.c_size_t * 6), ("off_reverselink", C.c_size_t)]


class SpawnLayout(C.Structure):
    _fields_ = [("off_id", C.c_size_t), ("off_mass", C.c_size_t), ("generation_shift", C.c_int), ("pad_", C.c_int)]


class BhParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("BoxSize", "ForceSoftening", "SeedBHDynMass", "atime", "a3inv", "hubble", "GravInternal", "BlackHoleAccretionFactor",
                                         "BlackHoleEddingtonFactor", "BlackHoleFeedbackFactor", "EddingtonConst", "UnitTime_in_s", "HubbleParam",
                                         "LightOverUnitVel", "MaxThermalU", "OmegaBaryon", "Hubble", "BHKE_EddingtonThrFactor", "BHKE_EddingtonMFactor",
                                         "BHKE_EddingtonMPivot", "BHKE_EddingtonMIndex", "BHKE_EffRhoFactor", "BHKE_EffCap", "BHKE_InjEnergyThr",
                                         "BHKE_SfrCritOverDensity")] + \
               [(k, C.c_int) for k in ("DensityKernelType", "WindsDecoupleSph", "RepositionEnabled", "MergeGravBound", "BH_DRAG", "BlackHoleKineticOn")]


class BhSlotView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64)] + \
               [(k, C.c_size_t) for k in ("off_mass", "off_mdot", "off_density", "off_mtrack", "off_dfaccel", "off_vdisp", "off_kineticfdbkenergy", "off_dragaccel",
                                          "off_encounter", "off_countprogs", "off_mintimebin", "off_swallowid", "off_swallowtime")]


class BhWork(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("SPH_SwallowID", "BH_SwallowID", "BH_FeedbackWeightSum", "BH_Entropy", "BH_SurroundingGasVel", "MgasEnc", "KEflag",
                                          "BH_accreted_Mass", "BH_accreted_BHMass", "BH_accreted_momentum")]


def bh_slot_view(arr):
    """shq_bh_slot_view of a numpy array of BH_DTYPE records"""
    f = BH_DTYPE.fields
    v = BhSlotView()
    v.base, v.elsize, v.numslots = arr.ctypes.data, BH_DTYPE.itemsize, len(arr)
    for key, name in (("off_mass", "Mass"), ("off_mdot", "Mdot"), ("off_density", "Density"), ("off_mtrack", "Mtrack"), ("off_dfaccel", "DFAccel"),
                      ("off_vdisp", "VDisp"), ("off_kineticfdbkenergy", "KineticFdbkEnergy"), ("off_dragaccel", "DragAccel"), ("off_encounter", "encounter"),
                      ("off_countprogs", "CountProgs"), ("off_mintimebin", "minTimeBin"), ("off_swallowid", "SwallowID"), ("off_swallowtime", "SwallowTime")):
        setattr(v, key, f[name][1])
    return v


class GasMetalView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64), ("off_density", C.c_size_t), ("off_metallicity", C.c_size_t),
                ("off_metals", C.c_size_t), ("nmetals", C.c_int), ("pad_", C.c_int)]


class WindParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("BoxSize", "Time", "WindFreeTravelLength", "MaxWindFreeTravelTime", "WindEfficiency", "WindSpeed", "WindSigma0",
                                         "WindSpeedFactor", "MinWindVelocity", "WindThermalFactor")] + [("WindModel", C.c_int), ("pad_", C.c_int)]


WIND_KICK_DTYPE = np.dtype([("part_index", "<i4"), ("pad_", "<i4"), ("StarDistance", "<f8"), ("StarID", "<u8"), ("StarKickVelocity", "<f8"), ("StarTherm", "<f8")])


class StarView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64), ("off_vdisp", C.c_size_t)]


class StarSpawnLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("star_formationtime", "star_lastenrichmentmyr", "star_totalmassreturned", "star_birthdensity", "star_vdisp",
                                         "star_metallicity", "star_metals", "sph_density", "sph_vdisp", "sph_metallicity", "sph_metals")] + [("nmetals", C.c_int), ("pad_", C.c_int)]


class BhSeedLayout(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("bh_mass", "bh_mseed", "bh_mdot", "bh_formationtime", "bh_swallowid", "bh_density", "bh_timebindynfric", "bh_minpotpos",
                                         "bh_dfaccel", "bh_df_surroundingvel", "bh_dragaccel", "bh_df_surroundingrmsvel", "bh_df_surroundingdensity", "bh_jumptominpot",
                                         "bh_countprogs", "bh_mtrack", "bh_kineticfdbkenergy", "bh_vdisp", "part_pos", "part_mass", "part_timebin_hydro")]


class ExchangeEntry(C.Structure):
    _fields_ = [("base", C.c_int64), ("slots", C.c_int64 * 6)]


# struct star_particle_data, libgadget/slotsmanager.h:77-92 (72 B)
STAR_DTYPE = np.dtype({"names": ["ReverseLink", "LastEnrichmentMyr", "TotalMassReturned", "Metallicity", "Metals", "VDisp", "BirthDensity", "FormationTime"],
                       "formats": ["<i4", "<f4", "<f8", "<f8", ("<f4", 9), "<f4", "<f4", "<f4"], "offsets": [0, 4, 8, 16, 24, 60, 64, 68], "itemsize": 72})


class FofParams(C.Structure):
    _fields_ = [("BoxSize", C.c_double), ("LinkingLength", C.c_double), ("PrimaryLinkTypes", C.c_int32), ("SecondaryLinkTypes", C.c_int32),
                ("HaloMinLength", C.c_int32), ("WindsDecoupleSph", C.c_int32)]


FOF_GROUP_DTYPE = np.dtype([("MinID", "<u8"), ("Length", "<i4"), ("GrNr", "<i4"), ("LenType", "<i4", 6), ("FirstPos", "<f4", 3), ("seed_index", "<i4"),
                            ("MassType", "<f8", 6), ("Mass", "<f8"), ("CM", "<f8", 3), ("Vel", "<f8", 3), ("Imom", "<f8", (3, 3)), ("Jmom", "<f8", 3),
                            ("MaxDens", "<f8"), ("first_member", "<i8")])


class TopNodeGeo(C.Structure):
    _fields_ = [("daughter", C.c_int32 * 8), ("leaf", C.c_int32), ("pad_", C.c_int32)]


class TopLeafMoments(C.Structure):
    _fields_ = [("s", C.c_double * 3), ("mass", C.c_double), ("hmax", C.c_double)]


TOPNODE_GEO_DTYPE = np.dtype([("daughter", "<i4", 8), ("leaf", "<i4"), ("pad_", "<i4")])
TOPLEAF_MOMENTS_DTYPE = np.dtype([("s", "<f8", 3), ("mass", "<f8"), ("hmax", "<f8")])


class Timeline(C.Structure):
    _fields_ = [("Ti_Current", C.c_int64), ("loga_now", C.c_double), ("Dloga_interval", C.c_double), ("nseg", C.c_int32), ("pad_", C.c_int32),
                ("seg_snap", C.c_int64 * 2), ("seg_loga", C.c_double * 3)]


class TimestepParams(C.Structure):
    _fields_ = [("ErrTolIntAccuracy", C.c_double), ("CourantFac", C.c_double), ("MinSizeTimestep", C.c_double), ("ForceSoftening", C.c_double),
                ("atime", C.c_double), ("hubble", C.c_double), ("fac3", C.c_double), ("dti_max", C.c_int64), ("ForceEqualTimesteps", C.c_int32),
                ("isFirstTimeStep", C.c_int32), ("mintimebin", C.c_int32), ("mingravtimebin", C.c_int32), ("tl", Timeline)]


class TimestepResult(C.Structure):
    _fields_ = [("badstepsizecount", C.c_int32), ("mTimeBin", C.c_int32), ("maxTimeBin", C.c_int32), ("mintimebin", C.c_int32),
                ("ntiaccel", C.c_int64), ("nticourant", C.c_int64), ("ntihsml", C.c_int64), ("ntiaccrete", C.c_int64), ("ntineighbour", C.c_int64),
                ("nbh", C.c_int64), ("dynratio", C.c_int64), ("maxdyndiff", C.c_int32), ("nbadbin", C.c_int32), ("dti_min", C.c_int64),
                ("timebincounts", C.c_int64 * (TIMEBINS + 1))]


class HierLevel(C.Structure):
    """shq_hier_level"""
    _fields_ = [("timebin", C.c_int32), ("walk_mode", C.c_int32), ("nparticles", C.c_int64), ("tree_nodes", C.c_int64),
                ("tree_build_ms", C.c_double), ("walk_ms", C.c_double)]


class DriftKickTimes(C.Structure):
    """DriftKickTimes, libgadget/timestep.h:10-26"""
    _fields_ = [("mintimebin", C.c_int), ("maxtimebin", C.c_int), ("mingravtimebin", C.c_int), ("Ti_kick", C.c_int64 * (TIMEBINS + 1)),
                ("Ti_lastactivedrift", C.c_int64 * (TIMEBINS + 1)), ("Ti_Current", C.c_int64), ("PM_length", C.c_int64), ("PM_start", C.c_int64),
                ("PM_kick", C.c_int64)]


class HostCosmo(C.Structure):
    _fields_ = [("OmegaBaryon", C.c_double), ("OmegaCDM", C.c_double), ("OmegaNu1", C.c_double), ("RhoCrit", C.c_double), ("Omega0", C.c_double),
                ("Hubble", C.c_double), ("GravInternal", C.c_double), ("hubble_now", C.c_double)]


class BhView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64),
                ("off_density", C.c_size_t), ("off_divvel", C.c_size_t)]


def sph_view(SphP):
    """shq_sph_view of a numpy array of SPH_DTYPE records."""
    v = SphView()
    f = SphP.dtype.fields
    v.base, v.elsize, v.numslots = SphP.ctypes.data, SphP.dtype.itemsize, len(SphP)
    v.off_density, v.off_egywtdensity, v.off_entropy = f["Density"][1], f["EgyWtDensity"][1], f["Entropy"][1]
    v.off_dtentropy, v.off_maxsignalvel, v.off_hydroaccel = f["DtEntropy"][1], f["MaxSignalVel"][1], f["HydroAccel"][1]
    v.off_dhsmlegydensityfactor, v.off_divvel, v.off_curlvel = f["DhsmlEgyDensityFactor"][1], f["DivVel"][1], f["CurlVel"][1]
    v.off_delaytime = f["DelayTime"][1]
    return v


def bh_view(BhP):
    v = BhView()
    f = BhP.dtype.fields
    v.base, v.elsize, v.numslots = BhP.ctypes.data, BhP.dtype.itemsize, len(BhP)
    v.off_density, v.off_divvel = f["Density"][1], f["DivVel"][1]
    return v


DENSITY_QUERY_DTYPE = np.dtype({"names": ["Pos", "NodeList", "Vel", "Hsml", "Type"], "formats": [("<f8", 3), ("<i4", 4), ("<f8", 3), "<f8", "<i4"],
                                "offsets": [0, 24, 40, 64, 72], "itemsize": 80})
DENSITY_RESULT_DTYPE = np.dtype([("EgyRho", "<f8"), ("DhsmlEgyDensity", "<f8"), ("Rho", "<f8"), ("DhsmlDensity", "<f8"), ("Ngb", "<f8"),
                                 ("Div", "<f8"), ("Rot", "<f8", 3), ("GradRho", "<f8", 3)])
HYDRO_QUERY_DTYPE = np.dtype({"names": ["Pos", "NodeList", "EgyRho", "EntVarPred", "Vel", "Hsml", "Mass", "Density", "Pressure", "F1",
                                        "SPH_DhsmlDensityFactor", "TimeBinHydro"],
                              "formats": [("<f8", 3), ("<i4", 4), "<f8", "<f8", ("<f8", 3), "<f8", "<f8", "<f8", "<f8", "<f8", "<f8", "<i4"],
                              "offsets": [0, 24, 40, 48, 56, 80, 88, 96, 104, 112, 120, 128], "itemsize": 136})
HYDRO_RESULT_DTYPE = np.dtype([("Acc", "<f8", 3), ("DtEntropy", "<f8"), ("MaxSignalVel", "<f8")])
assert DENSITY_RESULT_DTYPE.itemsize == 96 and HYDRO_RESULT_DTYPE.itemsize == 40


class StellarParams(C.Structure):
    _fields_ = [("BoxSize", C.c_double), ("DesNumNgb", C.c_double), ("MaxNgbDeviation", C.c_double), ("SPHWeighting", C.c_int32),
                ("DensityKernelType", C.c_int32)]


class SphStats(C.Structure):
    _fields_ = [("ntargets", C.c_int64), ("ninteractions", C.c_int64), ("niterations", C.c_int32), ("pad_", C.c_int32),
                ("kernel_ms", C.c_double), ("hsml_max_tried", C.c_double)]


class PMParams(C.Structure):
    _fields_ = [("Nmesh", C.c_int32), ("pad_", C.c_int32), ("BoxSize", C.c_double), ("Asmth", C.c_double),
                ("G", C.c_double)]


# ---- prototypes ------------------------------------------------------------------------------
_vp = C.c_void_p
hip.shq_last_error.restype = C.c_char_p
hip.shq_version.restype = C.c_char_p
hip.shq_init.argtypes = [C.c_int, _vp, C.POINTER(_vp)]
hip.shq_shutdown.argtypes = [_vp]
hip.shq_shutdown.restype = None
hip.shq_synchronize.argtypes = [_vp]
hip.shq_stream.argtypes = [_vp]
hip.shq_stream.restype = _vp
hip.shq_timer_begin.argtypes = [_vp, C.c_int]
hip.shq_timer_end.argtypes = [_vp, C.c_int]
hip.shq_timer_elapsed_ms.argtypes = [_vp, C.c_int, C.POINTER(C.c_double)]
hip.shq_particles_upload.argtypes = [_vp, C.POINTER(PartView)]
hip.shq_tree_upload.argtypes = [_vp, C.POINTER(TreeView)]
hip.shq_tree_build.argtypes = [_vp, C.c_double, C.c_int, _vp, C.c_int64, C.POINTER(TreeBuildStats)]
hip.shq_tree_build.restype = C.c_int
hip.shq_tree_download.argtypes = [_vp, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_int64)]
hip.shq_tree_download.restype = C.c_int
GRAV_QUERY_DTYPE = np.dtype({"names": ["Pos", "NodeList", "OldAcc"], "formats": [("<f8", 3), ("<i4", 4), "<f8"],
                             "offsets": [0, 24, 40], "itemsize": 48})
GRAV_RESULT_DTYPE = np.dtype({"names": ["Acc", "Potential"], "formats": [("<f8", 3), "<f8"], "offsets": [0, 24], "itemsize": 32})
hip.shq_grav_short_secondary.argtypes = [_vp, C.POINTER(GravParams), _vp, C.c_int64, _vp, _vp, C.c_int]
hip.shq_grav_short_secondary.restype = C.c_int
TOPLEAF_DTYPE = np.dtype([("Task", "<i4"), ("topnode", "<i4"), ("treenode", "<i4")])
DATA_INDEX_DTYPE = np.dtype([("Task", "<i4"), ("Index", "<i4"), ("NodeList", "<i4", 4)])
hip.shq_grav_reduce_export_results.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int]
hip.shq_grav_reduce_export_results.restype = C.c_int
hip.shq_grav_postprocess.argtypes = [_vp, C.POINTER(GravParams), _vp, C.c_int64, C.c_int]
hip.shq_grav_postprocess.restype = C.c_int
hip.shq_toptree_upload.argtypes = [_vp, C.POINTER(TreeView), _vp, C.c_int]
hip.shq_toptree_upload.restype = C.c_int
hip.shq_grav_toptree_exports.argtypes = [_vp, C.POINTER(GravParams), _vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_grav_toptree_exports.restype = C.c_int
hip.shq_ngb_toptree_exports.argtypes = [_vp, C.c_int, C.c_double, _vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_ngb_toptree_exports.restype = C.c_int
hip.shq_grav_toptree_exports_resident.argtypes = [_vp, C.POINTER(GravParams), _vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), _vp]
hip.shq_grav_toptree_exports_resident.restype = C.c_int
hip.shq_grav_export_pack.argtypes = [_vp, _vp, _vp]
hip.shq_grav_export_pack.restype = C.c_int
GAS_NCOL = 28
hip.shq_gas_set_device.argtypes = [_vp, _vp, C.c_int64, C.c_int64]
hip.shq_gas_get_device.argtypes = [_vp, _vp, C.c_int64, C.c_int]
hip.shq_density_resident.argtypes = [_vp, C.POINTER(DensityParams), C.POINTER(SphStats)]
hip.shq_hydro_resident.argtypes = [_vp, C.POINTER(HydroParams), C.POINTER(SphStats)]
for _f in ("shq_gas_set_device", "shq_gas_get_device", "shq_density_resident", "shq_hydro_resident"):
    getattr(hip, _f).restype = C.c_int
hip.shq_set_walk_stats.argtypes = [_vp, C.c_int]
hip.shq_set_walk_stats.restype = C.c_int
hip.shq_set_walk_launch.argtypes = [_vp, C.c_int, C.c_int]
hip.shq_set_walk_launch.restype = C.c_int
hip.shq_set_walk_sparse.argtypes = [_vp, C.c_int]
hip.shq_set_walk_sparse.restype = C.c_int
hip.shq_walk_pair_lean.argtypes = [_vp]
hip.shq_walk_pair_lean.restype = C.c_int
hip.shq_set_walk_overlap.argtypes = [_vp, C.c_int]
hip.shq_set_walk_overlap.restype = C.c_int
hip.shq_set_walk_addr.argtypes = [_vp, C.c_int]
hip.shq_set_walk_addr.restype = C.c_int
hip.shq_walk_last_addr.argtypes = [_vp, C.POINTER(C.c_int)]
hip.shq_walk_last_addr.restype = C.c_int
hip.shq_walk_addr32_fits.argtypes = [C.c_int64]
hip.shq_walk_addr32_fits.restype = C.c_int
hip.shq_pair_addr32_fits.argtypes = [C.c_int64, C.c_int64, C.c_int64]
hip.shq_pair_addr32_fits.restype = C.c_int
hip.shq_walk_last_pair_addr.argtypes = [_vp, C.POINTER(C.c_int)]
hip.shq_walk_last_pair_addr.restype = C.c_int
hip.shq_pm_set_fft_transposed.argtypes = [_vp, C.c_int]
hip.shq_pm_set_fft_transposed.restype = C.c_int
hip.shq_walk_pair_status.argtypes = [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.shq_walk_pair_status.restype = C.c_int
hip.shq_set_walk_debug.argtypes = [_vp, C.c_int, C.c_int]
hip.shq_set_walk_debug.restype = C.c_int
hip.shq_set_tree_debug.argtypes = [_vp, C.c_int64]
hip.shq_set_tree_debug.restype = C.c_int
hip.shq_tree_build_attempts.argtypes = [_vp, C.POINTER(C.c_int)]
hip.shq_tree_build_attempts.restype = C.c_int
hip.shq_direct_force_sample.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, _vp]
hip.shq_direct_force_sample.restype = C.c_int
hip.shq_exchange_plan.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp]
hip.shq_exchange_pack.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, _vp, C.c_int64, _vp, C.c_int, _vp, _vp]
hip.shq_exchange_unpack.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, C.c_int64, _vp, _vp, _vp, C.c_int]
hip.shq_slots_gc.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, C.POINTER(C.c_int64), C.c_int64, _vp, _vp, _vp]
hip.shq_slots_gc_sorted.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, C.POINTER(C.c_int64), C.c_int64, _vp, _vp, _vp]
hip.shq_slots_split_particles.argtypes = [_vp, C.POINTER(ExchangeLayout), C.POINTER(SpawnLayout), _vp, C.POINTER(C.c_int64), C.c_int64, _vp, _vp, C.c_int64, _vp]
hip.shq_slots_convert.argtypes = [_vp, C.POINTER(ExchangeLayout), _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64, C.c_int]
hip.shq_make_particle_stars.argtypes = [_vp, C.POINTER(ExchangeLayout), C.POINTER(StarSpawnLayout), _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double]
hip.shq_blackhole_make_seeds.argtypes = [_vp, C.POINTER(ExchangeLayout), C.POINTER(BhSeedLayout), _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int64,
                                         C.c_double, C.c_double]
hip.shq_bh_accretion.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhSlotView), _vp, _vp, C.c_int64, C.POINTER(KickFactors),
                                 C.POINTER(BhParams), C.c_int64, _vp, C.c_int64, C.POINTER(BhWork)]
hip.shq_bh_feedback.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhSlotView), _vp, _vp, C.c_int64, C.POINTER(KickFactors),
                                C.POINTER(BhParams), C.c_int64, _vp, C.c_int64, _vp, C.POINTER(BhWork), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.shq_bh_accretion.restype = hip.shq_bh_feedback.restype = C.c_int
# struct shq_bh_record: what a black-hole walk would have written on a neighbour, routed to the neighbour's owner.  One layout, read as
# a mark (the 8 bytes are the marking hole's ID) or as an effect (they are a double)
BH_MARK_DTYPE = np.dtype([("owner", "<i4"), ("part_index", "<i4"), ("hole", "<u4"), ("kind", "<i4"), ("id", "<u8")])
BH_EFFECT_DTYPE = np.dtype([("owner", "<i4"), ("part_index", "<i4"), ("hole", "<u4"), ("kind", "<i4"), ("value", "<f8")])
assert BH_MARK_DTYPE.itemsize == BH_EFFECT_DTYPE.itemsize == 24
_bh_dist = [C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_int64)]   # nlocal ... nrecords
hip.shq_bh_accretion_marks.argtypes = hip.shq_bh_accretion.argtypes + _bh_dist
hip.shq_bh_marks_resolve.argtypes = [_vp, C.POINTER(PartView), _vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(BhWork)]
hip.shq_bh_feedback_effects.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhSlotView), _vp, _vp, C.c_int64,
                                        C.POINTER(KickFactors), C.POINTER(BhParams), _vp, C.c_int64, C.POINTER(BhWork)] + _bh_dist
hip.shq_bh_effects_apply.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhSlotView), _vp, _vp, C.c_int64, C.POINTER(BhParams), C.c_int64, _vp,
                                     C.c_int64, _vp, C.POINTER(BhWork), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
for _f in ("shq_bh_accretion_marks", "shq_bh_marks_resolve", "shq_bh_feedback_effects", "shq_bh_effects_apply"):
    getattr(hip, _f).restype = C.c_int
hip.shq_winds_and_feedback.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(StarView), _vp, _vp, C.c_int64, C.POINTER(WindParams),
                                       _vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.shq_winds_and_feedback.restype = C.c_int
hip.shq_winds_candidates.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(StarView), _vp, _vp, C.c_int64, C.POINTER(WindParams),
                                     _vp, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_winds_apply.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), _vp, _vp, C.c_int64, C.POINTER(WindParams), _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_winds_candidates.restype = hip.shq_winds_apply.restype = C.c_int
hip.shq_metal_return.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(GasMetalView), _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _vp,
                                 C.POINTER(C.c_int64)]
hip.shq_metal_return.restype = C.c_int
# struct shq_metal_triple: a (gas particle, star, kernel weight) triple routed to the particle's owner
METAL_TRIPLE_DTYPE = np.dtype([("owner", "<i4"), ("part_index", "<i4"), ("star", "<u4"), ("pad_", "<i4"), ("wk", "<f8")])
METAL_STAR_NCOL = 12     # SHQ_METAL_STAR_NCOL: StarVolumeSPH, MassGenerated, MetalGenerated, MetalSpeciesGenerated[9]
hip.shq_metal_return_triples.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int64,
                                         _vp, C.c_int64, _vp, C.POINTER(C.c_int64)]
hip.shq_metal_return_apply.argtypes = [_vp, C.POINTER(PartView), C.POINTER(GasMetalView), _vp, C.c_int64, _vp, C.c_int64, C.c_double, _vp]
hip.shq_metal_return_sums.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp]
hip.shq_metal_return_triples.restype = hip.shq_metal_return_apply.restype = hip.shq_metal_return_sums.restype = C.c_int
hip.shq_domain_maintain_topleaf.argtypes = [_vp, C.c_int, C.c_int64, _vp, _vp, C.POINTER(C.c_int64)]
hip.shq_domain_maintain_topleaf.restype = C.c_int


# the domain decomposition (domain.hip): key tables, keys, samples, local top tree, serial stages, install, leaf counts, top leaves
class PeanoTables(C.Structure):
    _fields_ = [("nstates", C.c_int32), ("next", (C.c_uint8 * 8) * 64), ("sub", (C.c_uint8 * 8) * 64)]


class DomainParts(C.Structure):
    _fields_ = [("d_parts", C.c_void_p), ("elsize", C.c_size_t), ("off_flags", C.c_size_t), ("off_pos", C.c_size_t), ("numpart", C.c_int64), ("BoxSize", C.c_double)]


PEANO_KEYFN = C.CFUNCTYPE(C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int)
ERR_RETRY = 6
PEANOCELLS = 1 << 63
LOCAL_TOPNODE_DTYPE = np.dtype([("StartKey", "<u8"), ("Shift", "<i4"), ("Daughter", "<i4"), ("Parent", "<i4"), ("pad_", "<i4"), ("Count", "<i8"), ("Cost", "<i8")])
TOPNODE_DTYPE = np.dtype([("StartKey", "<u8"), ("Daughter", "<i4"), ("Shift", "<i4"), ("Leaf", "<i4"), ("pad_", "<i4")])
TOPLEAF_DTYPE = np.dtype([("Task", "<i4"), ("topnode", "<i4"), ("treenode", "<i4")])
TASK_LEAFS_DTYPE = np.dtype([("StartLeaf", "<i4"), ("EndLeaf", "<i4")])
hip.shq_peano_tables_from_key.argtypes = [_vp, C.POINTER(PeanoTables)]
hip.shq_peano_key_host.argtypes = [C.POINTER(PeanoTables), C.c_int, C.c_int, C.c_int, C.c_int]
hip.shq_peano_key_host.restype = C.c_uint64
hip.shq_peano_keys.argtypes = [_vp, C.POINTER(PeanoTables), _vp, C.c_size_t, C.c_int64, C.c_double, _vp]
hip.shq_domain_samples.argtypes = [_vp, C.POINTER(PeanoTables), C.POINTER(DomainParts), C.c_int, C.c_int, _vp, C.POINTER(C.c_int64)]
hip.shq_domain_local_toptree.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, _vp, C.POINTER(C.c_int)]
hip.shq_domain_toptree_merge.argtypes = [_vp, C.POINTER(C.c_int), _vp, C.c_int, C.c_int]
hip.shq_domain_toptree_finish.argtypes = [_vp, C.POINTER(C.c_int), C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.POINTER(C.c_int)]
hip.shq_domain_balance.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int64, C.c_double, _vp, C.POINTER(C.c_int)]
hip.shq_domain_install.argtypes = [_vp, C.POINTER(PeanoTables), _vp, C.c_int, _vp, C.c_int, _vp]
hip.shq_domain_leaf_counts.argtypes = [_vp, C.POINTER(DomainParts), _vp]
hip.shq_domain_particle_topleaves.argtypes = [_vp, C.POINTER(DomainParts), _vp, _vp]
for _f in ("shq_peano_tables_from_key", "shq_peano_keys", "shq_domain_samples", "shq_domain_local_toptree", "shq_domain_toptree_merge", "shq_domain_toptree_finish",
           "shq_domain_balance", "shq_domain_install", "shq_domain_leaf_counts", "shq_domain_particle_topleaves"):
    getattr(hip, _f).restype = C.c_int


def peano_tables_from_key(keyfn):
    """The key automaton of `keyfn` (a ctypes function pointer of the reference's signature, or a Python callable of (x, y, z, bits))."""
    cb = keyfn if isinstance(keyfn, C._CFuncPtr) else PEANO_KEYFN(keyfn)
    t = PeanoTables()
    check(hip.shq_peano_tables_from_key(C.cast(cb, C.c_void_p), C.byref(t)))
    return t


def peano_tables_to_arrays(t):
    n = int(t.nstates)
    return np.array([[t.next[s][o] for o in range(8)] for s in range(n)], dtype=np.uint8), np.array([[t.sub[s][o] for o in range(8)] for s in range(n)], dtype=np.uint8)


def peano_tables_from_arrays(nxt, sub):
    """PeanoTables from stored (next, sub) arrays of shape [nstates][8]"""
    t = PeanoTables()
    t.nstates = len(nxt)
    for s in range(len(nxt)):
        for o in range(8):
            t.next[s][o] = int(nxt[s][o])
            t.sub[s][o] = int(sub[s][o])
    return t
hip.shq_winds_evolve.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), _vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(KickFactors)]
hip.shq_winds_subgrid.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.c_size_t, _vp, _vp, C.c_int64, _vp, C.POINTER(WindParams), _vp, C.c_int64,
                                  C.POINTER(C.c_int64)]
hip.shq_winds_evolve.restype = hip.shq_winds_subgrid.restype = C.c_int
hip.shq_sph_state_upload.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView)]
hip.shq_sph_state_upload.restype = C.c_int
hip.shq_fof_group_sums.argtypes = [_vp, _vp, C.c_int, _vp]
hip.shq_fof_group_sums.restype = C.c_int
hip.shq_fof_seed_select.argtypes = [_vp, C.c_double, C.c_double, _vp, C.c_int64, C.POINTER(C.c_int64)]
for _f in ("shq_make_particle_stars", "shq_blackhole_make_seeds", "shq_fof_seed_select"):
    getattr(hip, _f).restype = C.c_int
for _f in ("shq_exchange_plan", "shq_exchange_pack", "shq_exchange_unpack", "shq_slots_gc", "shq_slots_gc_sorted", "shq_slots_split_particles", "shq_slots_convert"):
    getattr(hip, _f).restype = C.c_int
hip.shq_fof.argtypes = [_vp, C.POINTER(FofParams), _vp, _vp, _vp, C.POINTER(C.c_int64)]
hip.shq_fof.restype = C.c_int
hip.shq_fof_groups_download.argtypes = [_vp, _vp, C.c_int64]
hip.shq_fof_groups_download.restype = C.c_int
hip.shq_fof_members.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_fof_members.restype = C.c_int
hip.shq_tree_build_domain.argtypes = [_vp, C.c_double, C.c_int, _vp, C.c_int64, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int64, _vp, _vp]
hip.shq_tree_build_domain.restype = C.c_int
hip.shq_tree_set_topleaf_moments.argtypes = [_vp, _vp, C.c_int]
hip.shq_tree_set_topleaf_moments.restype = C.c_int
_tsp, _tsr = C.POINTER(TimestepParams), C.POINTER(TimestepResult)
hip.shq_find_timesteps.argtypes = [_vp, _tsp, _vp, C.c_int64, C.c_int64, C.c_int, _tsr]
hip.shq_find_global_timestep.argtypes = [_vp, _tsp, _tsr]
hip.shq_find_hydro_timesteps.argtypes = [_vp, _tsp, _vp, C.c_int64, _tsr]
hip.shq_set_bh_first_timestep.argtypes = [_vp, C.c_int]
hip.shq_hier_gravity_bins.argtypes = [_vp, _tsp, _vp, C.c_int64, C.c_int, C.c_int, _tsr]
hip.shq_hier_push_down.argtypes = [_vp, _vp, C.c_int64, C.c_int]
hip.shq_hier_refine.argtypes = [_vp, _tsp, _vp, C.c_int64, C.c_int, C.c_int, _tsr]
hip.shq_velocity_moments.argtypes = [_vp, _vp, _vp, _vp]
hip.shq_timebins_download.argtypes = [_vp, _vp, _vp]
hip.shq_maxsignalvel_upload.argtypes = [_vp, _vp]
hip.shq_bh_dynamics_upload.argtypes = [_vp, C.POINTER(PartView), C.POINTER(BhDynView)]
hip.shq_bh_dynamics_download.argtypes = [_vp, C.POINTER(PartView), C.POINTER(BhDynView)]
hip.shq_set_bh_reposition.argtypes = [_vp, C.c_int]
hip.shq_kick_bh.argtypes = [_vp, _vp, _vp, C.c_int64]
for _f in ("shq_find_timesteps", "shq_find_global_timestep", "shq_find_hydro_timesteps", "shq_set_bh_first_timestep", "shq_hier_gravity_bins",
           "shq_hier_push_down", "shq_hier_refine", "shq_velocity_moments", "shq_timebins_download", "shq_maxsignalvel_upload",
           "shq_bh_dynamics_upload", "shq_bh_dynamics_download", "shq_set_bh_reposition", "shq_kick_bh"):
    getattr(hip, _f).restype = C.c_int
hip.shq_pm_slab_pitch.argtypes = [C.c_int]
hip.shq_pm_slab_pitch.restype = C.c_int
hip.shq_pm_slab2_deposit.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_pm_slab2_deposit.restype = C.c_int
hip.shq_pm_slab2_deposit_ghosts.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_pm_slab2_deposit_ghosts.restype = C.c_int
hip.shq_set_inputs_current.argtypes = [_vp, C.c_int]
hip.shq_set_inputs_current.restype = C.c_int
CURRENT_PARTICLES, CURRENT_SPH, CURRENT_TREE, CURRENT_IDS = 1, 2, 4, 8
hip.shq_pm_slab2_fft_yz.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int]
hip.shq_pm_slab2_fft_yz_packed.argtypes = [_vp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
hip.shq_pm_slab2_fft_yz_packed.restype = C.c_int
hip.shq_pm_slab2_fft_yz.restype = C.c_int
hip.shq_pm_slab2_xgreen.argtypes = [_vp, C.POINTER(PMParams), _vp, C.c_int, C.c_int]
hip.shq_pm_slab2_xgreen.restype = C.c_int
hip.shq_pm_slab2_xforward.argtypes = [_vp, C.POINTER(PMParams), _vp, C.c_int, C.c_int]
hip.shq_pm_slab2_xforward.restype = C.c_int
hip.shq_pm_slab2_xfinish.argtypes = [_vp, C.POINTER(PMParams), _vp, C.c_int, C.c_int, _vp]
hip.shq_pm_slab2_xfinish.restype = C.c_int
hip.shq_pm_slab_xforward.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, _vp]
hip.shq_pm_slab_xforward.restype = C.c_int
hip.shq_pm_slab_xfinish.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, _vp, _vp]
hip.shq_pm_slab_xfinish.restype = C.c_int
hip.shq_particles_set_device_types.argtypes = [_vp, _vp, C.c_int64]
hip.shq_particles_set_device_types.restype = C.c_int
hip.shq_pm_slab2_readout.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_pm_slab2_readout.restype = C.c_int
hip.shq_pm_measure_power.argtypes = [_vp, C.c_int]
hip.shq_pm_measure_power.restype = C.c_int
hip.shq_pm_get_measure_power.argtypes = [_vp]
hip.shq_pm_get_measure_power.restype = C.c_int
hip.shq_pm_download_power.argtypes = [_vp, C.c_int, _vp, _vp, _vp, _vp]
hip.shq_pm_download_power.restype = C.c_int
hip.shq_dynamics_upload.argtypes = [_vp, C.POINTER(PartView)]
hip.shq_dynamics_upload.restype = C.c_int
hip.shq_drift.argtypes = [_vp, C.c_double, C.c_double, _vp]
hip.shq_drift.restype = C.c_int
hip.shq_kick_short.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int]
hip.shq_kick_short.restype = C.c_int
hip.shq_timebins_upload.argtypes = [_vp, _vp, _vp]
hip.shq_timebins_upload.restype = C.c_int
hip.shq_build_active_particles.argtypes = [_vp, C.c_int64, C.c_int, C.POINTER(ActiveInfo)]
hip.shq_build_active_particles.restype = C.c_int
hip.shq_build_active_sublist.argtypes = [_vp, C.c_int, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_build_active_sublist.restype = C.c_int
hip.shq_hier_gravity_levels.argtypes = [_vp, _tsp, C.POINTER(GravParams), C.c_double, C.c_int, C.c_int64, C.c_int, _vp, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int64), C.POINTER(HierLevel), C.POINTER(C.c_int)]
hip.shq_hier_gravity_levels.restype = C.c_int
hip.shq_active_download.argtypes = [_vp, C.c_int, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_active_download.restype = C.c_int
hip.shq_kick_hydro.argtypes = [_vp, _vp, _vp, C.c_double, C.c_double, _vp, C.c_int64, C.c_int, C.POINTER(C.c_int64)]
hip.shq_kick_hydro.restype = C.c_int
hip.shq_entropy_download.argtypes = [_vp, _vp]
hip.shq_entropy_download.restype = C.c_int
hip.shq_kick_pm.argtypes = [_vp, C.c_double]
hip.shq_kick_pm.restype = C.c_int
hip.shq_dynamics_download.argtypes = [_vp, C.POINTER(PartView)]
hip.shq_dynamics_download.restype = C.c_int
hip.shq_grav_short_run.argtypes = [_vp, C.POINTER(GravParams), _vp, C.c_int64, C.c_int, C.c_int]
hip.shq_grav_short_run_range.argtypes = [_vp, C.POINTER(GravParams), C.c_int64, C.c_int64, C.c_int, C.c_int]
hip.shq_hilbert_order.argtypes = [_vp, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
hip.shq_grav_short_download.argtypes = [_vp, _vp, _vp, _vp, C.POINTER(WalkStats)]
hip.shq_grav_refresh_oldacc.argtypes = [_vp, C.c_double]
hip.shq_grav_short_tree.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), _vp, C.c_int64,
                                    C.POINTER(GravParams), _vp, C.c_int, C.c_int, C.POINTER(WalkStats)]
hip.shq_pm_force.argtypes = [_vp, C.POINTER(PMParams), C.POINTER(PartView), _vp, _vp]
hip.shq_pm_run.argtypes = [_vp, C.POINTER(PMParams)]
hip.shq_pm_download.argtypes = [_vp, _vp, _vp]
hip.shq_treepm_step.argtypes = [_vp, C.POINTER(PMParams), C.POINTER(GravParams), C.c_int, C.c_int]
class PMTransfer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("zero_mode", C.c_int32), ("pad_", C.c_int32), ("table", C.c_void_p)]


hip.shq_pm_apply.argtypes = [_vp, C.c_int, _vp, C.POINTER(PMTransfer), _vp]
hip.shq_pm_apply.restype = C.c_int
hip.shq_timer_between_ms.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
hip.shq_timer_between_ms.restype = C.c_int
hip.shq_pm_start.argtypes = [_vp, _vp, C.c_double]
hip.shq_pm_start.restype = C.c_int
hip.shq_pm_forward.argtypes = [_vp, C.POINTER(PMParams)]
hip.shq_pm_forward.restype = C.c_int
hip.shq_pm_set_mode_factor.argtypes = [_vp, C.c_int, _vp]
hip.shq_pm_set_mode_factor.restype = C.c_int
hip.shq_pm_set_deposit_types.argtypes = [_vp, C.c_int]
hip.shq_pm_set_deposit_types.restype = C.c_int
ALL_TYPES = -1                                     # SHQ_ALL_TYPES


class UvbgParams(C.Structure):
    """shq_uvbg_params: UVBGParams (uvbg.cpp:32-56) plus the mesh's BoxSize"""
    _fields_ = [
        ("ReionRBubbleMax", C.c_double), ("ReionRBubbleMin", C.c_double), ("ReionDeltaRFactor", C.c_double),
        ("ReionFilterType", C.c_int32), ("RtoMFilterType", C.c_int32),
        ("ReionGammaHaloBias", C.c_double), ("ReionNionPhotPerBary", C.c_double), ("AlphaUV", C.c_double),
        ("EscapeFractionNorm", C.c_double), ("EscapeFractionScaling", C.c_double),
        ("ReionUseParticleSFR", C.c_int32), ("pad0_", C.c_int32), ("ReionSFRTimescale", C.c_double),
        ("UVBGdim", C.c_int32), ("pad1_", C.c_int32), ("BoxSize", C.c_double),
    ]


class UvbgCosmo(C.Structure):
    """shq_uvbg_cosmo: Time, the cosmology's scalars, hubble_function(CP, Time) and the units"""
    _fields_ = [(f, C.c_double) for f in ("Time", "Omega0", "OmegaBaryon", "RhoCrit", "HubbleParam", "hubble",
                                          "UnitLength_in_cm", "UnitMass_in_g", "UnitTime_in_s")]


class UvbgResult(C.Structure):
    _fields_ = [("volume_weighted_global_xHI", C.c_double), ("mass_weighted_global_xHI", C.c_double),
                ("nradii", C.c_int32), ("pad_", C.c_int32)]


hip.shq_uvbg_calculate.argtypes = [_vp, C.POINTER(UvbgParams), C.POINTER(UvbgCosmo), C.POINTER(PartView), _vp, _vp, _vp, _vp,
                                   C.POINTER(UvbgResult)]
hip.shq_uvbg_calculate.restype = C.c_int
hip.shq_uvbg_keep_grids.argtypes = [_vp, C.c_int]
hip.shq_uvbg_keep_grids.restype = C.c_int
hip.shq_uvbg_download_grids.argtypes = [_vp, C.c_int, _vp, _vp]
hip.shq_uvbg_download_grids.restype = C.c_int
hip.shq_uvbg_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 4)]
hip.shq_uvbg_phase_ms.restype = C.c_int
hip.shq_uvbg_filter_table.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, _vp]
hip.shq_uvbg_filter_table.restype = C.c_int
# the phases on a rank's x-slab (dist.DistUVBG): device pointers of torch tensors
_UP, _UC = C.POINTER(UvbgParams), C.POINTER(UvbgCosmo)
hip.shq_uvbg_slab_pitch.argtypes = [C.c_int]
hip.shq_uvbg_slab_fesc.argtypes = [_vp, _UP, _UC, _vp, _vp, C.c_int64, _vp, _vp, C.POINTER(C.c_double * 3), C.POINTER(C.c_int)]
hip.shq_uvbg_slab_deposit.argtypes = [_vp, _UP, _vp, _vp, C.c_int64, _vp, _vp, C.POINTER(C.c_int * 3)] + [C.c_int] * 5 + [_vp] * 3
hip.shq_uvbg_slab_fft_yz.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int]
hip.shq_uvbg_slab_xforward.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int]
hip.shq_uvbg_slab_tables.argtypes = [_vp, C.c_int, C.c_int, C.c_double, _vp, C.c_int]
hip.shq_uvbg_slab_xfilter.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_uvbg_slab_filter.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_uvbg_slab_cells.argtypes = [_vp, _UP, _UC, C.c_double, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                    C.POINTER(C.c_double * 3)]
hip.shq_uvbg_slab_readout.argtypes = [_vp, _UP, _UC, _vp, _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]
for _f in ("pitch", "fesc", "deposit", "fft_yz", "xforward", "tables", "xfilter", "filter", "cells", "readout"):
    getattr(hip, "shq_uvbg_slab_" + _f).restype = C.c_int


FLAG_HEIII = 4                                     # SHQ_FLAG_HEIII: HeIIIionized, bit 2 of the flag byte


class HeiiiParams(C.Structure):
    """shq_heiii_params: QSOLightupParams, the history's target and Q_inst at this step, units, cosmology and the particle offset"""
    _fields_ = [(f, C.c_double) for f in ("BoxSize", "atime", "qso_candidate_min_mass", "qso_candidate_max_mass", "mean_bubble",
                                          "var_bubble", "heIIIreion_finish_frac", "desired_ion_frac", "qso_inst_heating", "uu_in_cgs",
                                          "OmegaBaryon", "HubbleParam")] + [("CurrentParticleOffset", C.c_double * 3), ("n_gas_tot", C.c_int64)]


HEIII_QUASAR_DTYPE = np.dtype([("group", "<i4"), ("pad_", "<i4"), ("pos", "<f8", 3), ("ionfrac", "<f8"), ("n_ionized", "<i8")])


class HeiiiResult(C.Structure):
    _fields_ = [("init_ionfrac", C.c_double), ("final_ionfrac", C.c_double), ("n_candidates", C.c_int64), ("n_iterations", C.c_int64),
                ("n_flash", C.c_int64), ("n_ionized", C.c_int64)]


HEIII_NSTAT = 32


class HeiiiStats(C.Structure):
    _fields_ = [("ms", C.c_double * 4), ("nsweeps", C.c_int64), ("ndraws", C.c_int64), ("nbubbles", C.c_int64), ("neligible", C.c_int64),
                ("ntests", C.c_int64), ("sweep_draws", C.c_int32 * HEIII_NSTAT), ("sweep_lit", C.c_int32 * HEIII_NSTAT),
                ("sweep_eligible", C.c_int64 * HEIII_NSTAT)]


hip.shq_heiii_reionization.argtypes = [_vp, C.POINTER(HeiiiParams), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(TreeView), _vp,
                                       C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(HeiiiResult)]
hip.shq_heiii_reionization.restype = C.c_int
hip.shq_heiii_last_stats.argtypes = [_vp, C.POINTER(HeiiiStats)]
hip.shq_heiii_last_stats.restype = C.c_int

# the operator in phases (open / sweep / commit / close), for DistHeIII
HEIII_BUBBLE_DTYPE = np.dtype([("c", "<f8", 3), ("R", "<f8"), ("seq", "<i4"), ("pad_", "<i4")])   # shq_heiii_bubble
HEIII_MAX_SEQ = 1024
hip.shq_heiii_open.argtypes = [_vp, C.POINTER(HeiiiParams), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                               C.POINTER(C.c_int64), _vp, _vp]
hip.shq_heiii_sweep.argtypes = [_vp, _vp, C.c_int, C.c_int, _vp]
hip.shq_heiii_commit.argtypes = [_vp, C.c_int, C.POINTER(C.c_int64)]
hip.shq_heiii_close.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(C.c_int64)]
hip.shq_heiii_host_numbers.argtypes = [C.POINTER(HeiiiParams), _vp, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_int64)]
for _f in ("open", "sweep", "commit", "close", "host_numbers"):
    getattr(hip, "shq_heiii_" + _f).restype = C.c_int


class LensParams(C.Structure):
    """shq_lens_params: PlaneParams (plane.cpp:25-33) for one call, the box and the particle offset"""
    _fields_ = [("Resolution", C.c_int32), ("ncuts", C.c_int32), ("nnormals", C.c_int32), ("exclude_type2", C.c_int32),
                ("CutPoints", C.c_void_p), ("Normals", C.c_void_p), ("Thickness", C.c_double), ("BoxSize", C.c_double),
                ("CurrentParticleOffset", C.c_double * 3)]


class LensCosmo(C.Structure):
    _fields_ = [("atime", C.c_double), ("comoving_distance", C.c_double), ("HubbleParam", C.c_double), ("omega_source", C.c_double),
                ("num_particles_tot", C.c_int64)]


class LensNuMesh(C.Structure):
    """shq_lens_numesh: the rank's x-slab [x0, x0 + nx) of the PM neutrino correction mesh, dense [nx][Nmesh][Nmesh]"""
    _fields_ = [("Nmesh", C.c_int32), ("x0", C.c_int32), ("nx", C.c_int32), ("pad_", C.c_int32), ("inv_fft_norm", C.c_double),
                ("mean_mass_cell", C.c_double), ("real", C.c_void_p)]


hip.shq_lens_count_active.argtypes = [_vp, C.POINTER(PartView), C.c_int, C.POINTER(C.c_int64)]
hip.shq_lens_count_active.restype = C.c_int
hip.shq_lens_num_cuts.argtypes = [C.POINTER(LensParams), C.POINTER(C.c_int32)]
hip.shq_lens_num_cuts.restype = C.c_int
hip.shq_lens_planes.argtypes = [_vp, C.POINTER(LensParams), C.POINTER(LensCosmo), C.POINTER(PartView), C.POINTER(LensNuMesh), _vp, _vp, _vp]
hip.shq_lens_planes.restype = C.c_int
hip.shq_lens_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 4)]
hip.shq_lens_phase_ms.restype = C.c_int


class ZeldovichParams(C.Structure):
    """shq_zeldovich_params: what displacement_fields reads of GenicConfig, and the caller's vel_prefac"""
    _fields_ = [("Nmesh", C.c_int32), ("Seed", C.c_int32), ("UnitaryAmplitude", C.c_int32), ("InvertPhase", C.c_int32),
                ("ScaleDepVelocity", C.c_int32), ("pad_", C.c_int32), ("BoxSize", C.c_double), ("vel_prefac", C.c_double)]


hip.shq_zeldovich_seed_table.argtypes = [C.c_int, C.c_int, _vp, _vp]
hip.shq_zeldovich_seed_table.restype = C.c_int
hip.shq_zeldovich_factor_tables.argtypes = [C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp]
hip.shq_zeldovich_factor_tables.restype = C.c_int
hip.shq_zeldovich_fill.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int]
hip.shq_zeldovich_fill.restype = C.c_int
hip.shq_zeldovich_download_field.argtypes = [_vp, C.c_int, _vp]
hip.shq_zeldovich_download_field.restype = C.c_int
hip.shq_zeldovich_drop_field.argtypes = [_vp]
hip.shq_zeldovich_drop_field.restype = C.c_int
hip.shq_zeldovich_set_fill_chunk.argtypes = [_vp, C.c_int64]
hip.shq_zeldovich_set_fill_chunk.restype = C.c_int
hip.shq_zeldovich_displacements.argtypes = [_vp, C.POINTER(ZeldovichParams), _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double)]
hip.shq_zeldovich_displacements.restype = C.c_int
hip.shq_zeldovich_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 4)]
hip.shq_zeldovich_phase_ms.restype = C.c_int
hip.shq_zeldovich_column_draws.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]
hip.shq_zeldovich_column_draws.restype = C.c_int
hip.shq_zeldovich_slab_pitch.argtypes = [C.c_int]
hip.shq_zeldovich_slab_fill.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_zeldovich_slab_tables.argtypes = [_vp, C.c_int, C.c_double, _vp, _vp]
hip.shq_zeldovich_slab_xtransfer.argtypes = [_vp, C.c_int, C.c_double, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_zeldovich_slab_transfer.argtypes = [_vp, C.c_int, C.c_double, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_zeldovich_slab_fft_yz.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int]
hip.shq_zeldovich_slab_gather.argtypes = [_vp, C.c_int, C.c_double, _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_zeldovich_slab_finalize.argtypes = [_vp, C.c_int64, _vp, _vp, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp, C.POINTER(C.c_double * 2)]
for _f in ("pitch", "fill", "tables", "xtransfer", "transfer", "fft_yz", "gather", "finalize"):
    getattr(hip, "shq_zeldovich_slab_" + _f).restype = C.c_int


class GlassParams(C.Structure):
    """shq_glass_params"""
    _fields_ = [("Nmesh", C.c_int32), ("nsteps", C.c_int32), ("BoxSize", C.c_double)]


class GlassStep(C.Structure):
    """shq_glass_step: the times and glass_stats of one step"""
    _fields_ = [("t_f", C.c_double), ("t_v", C.c_double), ("t_x", C.c_double), ("force_std", C.c_double), ("vel_std", C.c_double)]


hip.shq_glass_evolve.argtypes = [_vp, C.POINTER(GlassParams), C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
hip.shq_glass_evolve.restype = C.c_int
hip.shq_glass_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 4)]
hip.shq_glass_phase_ms.restype = C.c_int
hip.shq_glass_setup_positions.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, _vp]
hip.shq_glass_setup_positions.restype = C.c_int
hip.shq_glass_finish_power.argtypes = [C.c_int, C.c_double, _vp, _vp, _vp, C.c_double, C.POINTER(C.c_int)]
hip.shq_glass_finish_power.restype = C.c_int
hip.shq_glass_setup_positions_block.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int * 2), C.POINTER(C.c_int * 2), _vp]
hip.shq_glass_setup_positions_block.restype = C.c_int
hip.shq_glass_slab_pitch.argtypes = [C.c_int]
hip.shq_glass_slab_tables.argtypes = [_vp, C.c_int, C.c_double, C.c_double]
hip.shq_glass_slab_planes.argtypes = [_vp, C.c_int, C.c_double, _vp, C.c_int64, _vp]
hip.shq_glass_slab_deposit.argtypes = [_vp, C.c_int, C.c_double, _vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
hip.shq_glass_slab_fft_yz.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int]
hip.shq_glass_slab_xforward.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp]
hip.shq_glass_slab_xtransfer.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_glass_slab_power.argtypes = [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp]
hip.shq_glass_slab_transfer.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]
hip.shq_glass_slab_gather.argtypes = [_vp, C.c_int, C.c_double, _vp, C.c_int64, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int]
hip.shq_glass_slab_particles.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_double * 2)]
for _f in ("pitch", "tables", "planes", "deposit", "fft_yz", "xforward", "xtransfer", "power", "transfer", "gather", "particles"):
    getattr(hip, "shq_glass_slab_" + _f).restype = C.c_int

THERMAL_NKNOTS = 2000


class ThermalParams(C.Structure):
    """shq_thermal_params: the lattice, the rank's sub-block of columns and thermalvel.m_vamp"""
    _fields_ = [("Ngrid", C.c_int32), ("x0", C.c_int32), ("nx", C.c_int32), ("y0", C.c_int32), ("ny", C.c_int32), ("pad_", C.c_int32),
                ("v_amp", C.c_double)]


hip.shq_thermal_seed_table.argtypes = [C.c_int, C.c_int, _vp]
hip.shq_thermal_seed_table.restype = C.c_int
hip.shq_thermal_tables.argtypes = [C.c_double, C.c_double, _vp, _vp, C.POINTER(C.c_double)]
hip.shq_thermal_tables.restype = C.c_int
hip.shq_thermal_speeds.argtypes = [_vp, C.POINTER(ThermalParams), _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]
hip.shq_thermal_speeds.restype = C.c_int
hip.shq_thermal_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 3)]
hip.shq_thermal_phase_ms.restype = C.c_int
hip.shq_thermal_column_draws.argtypes = [_vp, C.c_int, _vp, C.c_int, _vp]
hip.shq_thermal_column_draws.restype = C.c_int


class YieldTables(C.Structure):
    """shq_yield_tables: the caller's lifetime / AGB / SNII / SN Ia tables, laid out value[mass index * nmet + metallicity index]"""
    _fields_ = [("life_nmet", C.c_int32), ("life_nmass", C.c_int32), ("lifetime_metallicity", _vp), ("lifetime_masses", _vp), ("lifetime", _vp),
                ("agb_nmet", C.c_int32), ("agb_nmass", C.c_int32), ("agb_metallicities", _vp), ("agb_masses", _vp), ("agb_total_mass", _vp),
                ("agb_total_metals", _vp), ("agb_yield", _vp),
                ("snii_nmet", C.c_int32), ("snii_nmass", C.c_int32), ("snii_metallicities", _vp), ("snii_masses", _vp), ("snii_total_mass", _vp),
                ("snii_total_metals", _vp), ("snii_yield", _vp),
                ("nmetals", C.c_int32), ("pad_", C.c_int32), ("sn1a_total_metals", C.c_double), ("sn1a_yields", _vp)]


class CosmicTimeTable(C.Structure):
    """shq_cosmic_time_table"""
    _fields_ = [("n", C.c_int64), ("loga0", C.c_double), ("dloga", C.c_double), ("T", _vp), ("dTdloga", _vp)]


class YieldParams(C.Structure):
    """shq_yield_params"""
    _fields_ = [(k, C.c_double) for k in ("Sn1aN0", "HubbleParam", "imf_norm", "MAXMASS", "SNAGBSWITCH")]


class StarYieldView(C.Structure):
    """shq_star_yield_view"""
    _fields_ = [("base", C.c_void_p), ("elsize", C.c_size_t), ("numslots", C.c_int64), ("off_formationtime", C.c_size_t),
                ("off_lastenrichmentmyr", C.c_size_t), ("off_totalmassreturned", C.c_size_t), ("off_metallicity", C.c_size_t)]


def star_yield_view(StarP):
    f = StarP.dtype.fields
    return StarYieldView(StarP.ctypes.data, StarP.dtype.itemsize, len(StarP), f["FormationTime"][1], f["LastEnrichmentMyr"][1],
                         f["TotalMassReturned"][1], f["Metallicity"][1])


hip.shq_yields_init.argtypes = [_vp, C.POINTER(YieldTables), C.POINTER(CosmicTimeTable), C.POINTER(YieldParams), C.POINTER(C.c_double)]
hip.shq_yields_init.restype = C.c_int
hip.shq_metal_yields.argtypes = [_vp, C.POINTER(PartView), C.POINTER(StarYieldView), _vp, C.c_int64, C.c_double, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int64),
                                 _vp, _vp, _vp, C.POINTER(C.c_int64)]
hip.shq_metal_yields.restype = C.c_int
hip.shq_metal_return_postprocess.argtypes = [_vp, C.POINTER(PartView), C.POINTER(StarYieldView), _vp, C.c_int64, _vp, _vp]
hip.shq_metal_return_postprocess.restype = C.c_int
hip.shq_metal_yields_last_ms.argtypes = [_vp, C.POINTER(C.c_double * 2)]
hip.shq_metal_yields_last_ms.restype = C.c_int

# ---- radiative cooling -------------------------------------------------------------------------
COOL_OK, COOL_DEFERRED, COOL_BADINPUT, COOL_NOCONV = 0, 1, 2, 3
COOL_WHAT = {"UNEW": 0, "TCOOL": 1, "NH0": 2, "HE0": 3, "HEP": 4, "HEPP": 5, "TEMP": 6, "LAMBDANET": 7}
COOL_UVBG_GLOBAL, COOL_UVBG_ZREION, COOL_UVBG_J21 = 0, 1, 2


class CoolingUVBG(C.Structure):
    """shq_cooling_uvbg (struct UVBG)"""
    _fields_ = [(k, C.c_double) for k in ("J_UV", "gJH0", "gJHep", "gJHe0", "epsH0", "epsHep", "epsHe0", "self_shield_dens", "zreion")]


class CoolingTables(C.Structure):
    """shq_cooling_tables"""
    _fields_ = [("rate_tables", _vp), ("cooling", C.c_int32), ("SelfShieldingOn", C.c_int32), ("HeliumHeatOn", C.c_int32), ("pad_", C.c_int32),
                ("MinGasTemp", C.c_double), ("CMBTemperature", C.c_double), ("HeliumHeatThresh", C.c_double), ("HeliumHeatAmp", C.c_double),
                ("HeliumHeatExp", C.c_double), ("rho_crit_baryon", C.c_double), ("fBar", C.c_double),
                ("density_in_phys_cgs", C.c_double), ("uu_in_cgs", C.c_double), ("tt_in_s", C.c_double),
                ("metal", _vp), ("metal_dims", C.c_int32 * 3), ("pad2_", C.c_int32), ("metal_min", C.c_double * 3), ("metal_max", C.c_double * 3),
                ("zreion", _vp), ("zreion_nside", C.c_int32), ("pad3_", C.c_int32), ("zreion_boxsize", C.c_double)]


class CoolingFields(C.Structure):
    """shq_cooling_fields"""
    _fields_ = [("off_ne", C.c_size_t), ("off_metallicity", C.c_size_t), ("off_sfr", C.c_size_t), ("off_delaytime", C.c_size_t)]


class CoolingStep(C.Structure):
    """shq_cooling_step"""
    _fields_ = [("redshift", C.c_double), ("a3inv", C.c_double), ("hubble", C.c_double), ("kf", KickFactors),
                ("lastred_for_bin", C.c_double * (TIMEBINS + 1)), ("GlobalUVBG", CoolingUVBG), ("uvbg_mode", C.c_int32), ("StarformationOn", C.c_int32),
                ("HIReionTemp", C.c_double), ("temp_to_u", C.c_double), ("MinGasTemp", C.c_double), ("lmfp_heat", C.c_double),
                ("CurrentParticleOffset", C.c_double * 3), ("PhysDensThresh", C.c_double), ("OverDensThresh", C.c_double),
                ("local_J21", _vp), ("zreion", _vp), ("J21_coeffs", C.c_double * 6), ("ss_greyopac_factor", C.c_double), ("ss_fbar_factor", C.c_double)]


class CoolingResult(C.Structure):
    """shq_cooling_result"""
    _fields_ = [("n_status", C.c_int64 * 4), ("n_skipped", C.c_int64), ("n_eeqos", C.c_int64), ("n_deferred", C.c_int64), ("steps", C.c_int64),
                ("kernel_ms", C.c_double)]


hip.shq_cooling_set_tables.argtypes = [_vp, C.POINTER(CoolingTables)]
hip.shq_cooling_set_refill.argtypes = [_vp, C.c_int]
_cool_eval_tail = [C.c_int, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(CoolingUVBG), C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]
hip.shq_cooling_eval.argtypes = [_vp] + _cool_eval_tail
hip.shq_cooling_eval_host.argtypes = [C.POINTER(CoolingTables)] + _cool_eval_tail + [C.c_int]
hip.shq_cooling.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(CoolingFields), _vp, C.c_int64, C.POINTER(CoolingStep), _vp, _vp, C.c_int64,
                            _vp, C.c_int64, C.POINTER(CoolingResult)]
hip.shq_cooling_last_kernel.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
for _f in ("shq_cooling_set_tables", "shq_cooling_set_refill", "shq_cooling_eval", "shq_cooling_eval_host", "shq_cooling", "shq_cooling_last_kernel"):
    getattr(hip, _f).restype = C.c_int

# ---- star formation on the effective equation of state -----------------------------------------
SFR_WHAT = {"STARFORM": 0, "EGYEFF": 1, "NH0": 2, "HE0": 3, "HEP": 4, "HEPP": 5, "ON_EEQOS": 6}
SFR_OUT = ("trelax", "tsfr", "egyhot", "egycold", "cloudfrac", "ne_eeqos", "smr", "sm", "dM", "Sfr", "Ne", "Metallicity", "Entropy", "mass_of_star", "prob",
           "query", "egyeff4", "tcool_relax", "egyeff", "egycurrent", "trelax_used", "dtime", "factorEVP", "densityfac", "frac")
SFR_NONE, SFR_CONVERT, SFR_SPLIT = 0, 1, 2
SFR_B_ON_EEQOS, SFR_B_CLAUSE4, SFR_B_TCOOL, SFR_B_TCOOL_WON, SFR_B_STAR, SFR_B_RELAXED = 1, 2, 4, 8, 16, 32
SFR_FLAG_BHHEATED = 8


class SfrParams(C.Structure):
    """shq_sfr_params"""
    _fields_ = [(k, C.c_int32) for k in ("StarformationCriterion", "BHFeedbackUseTcool", "Generations", "BoostSFDenseGas", "winds_subgrid", "pad_")] + \
               [(k, C.c_double) for k in ("PhysDensThresh", "OverDensThresh", "EgySpecSN", "EgySpecCold", "FactorSN", "FactorEVP", "MaxSfrTimescale", "tau_fmol_unit",
                                          "QuickLymanAlphaProbability", "QuickLymanAlphaTempThresh", "avg_baryon_mass", "temp_to_u", "UnitSfr_in_solar_per_year",
                                          "BoostSFOverDenseFactor", "GravInternal")]


SFR_ARRAYS = ("Density", "Entropy", "Ne", "Metallicity", "Mass", "Hsml", "DivVel", "CurlVel", "GradRho", "dloga", "DelayTime", "timebin", "flags", "ID")


class SfrArrays(C.Structure):
    """shq_sfr_arrays"""
    _fields_ = [(k, _vp) for k in SFR_ARRAYS]


class SfrEvalStep(C.Structure):
    """shq_sfr_eval_step"""
    _fields_ = [("redshift", C.c_double), ("a3inv", C.c_double), ("hubble", C.c_double), ("GlobalUVBG", CoolingUVBG), ("LocalUVBG", CoolingUVBG),
                ("rnd_table", _vp), ("rnd_size", C.c_int64)]


class SfrFields(C.Structure):
    """shq_sfr_fields"""
    _fields_ = [("off_ne", C.c_size_t), ("off_metallicity", C.c_size_t), ("off_sfr", C.c_size_t), ("off_delaytime", C.c_size_t)]


class SfrResultC(C.Structure):
    """shq_sfr_result"""
    _fields_ = [("n_status", C.c_int64 * 4), ("n_skipped", C.c_int64), ("n_newstars", C.c_int64), ("n_split", C.c_int64), ("n_maybewind", C.c_int64),
                ("n_deferred", C.c_int64), ("sum_sf_part", C.c_int64), ("localsfr", C.c_double), ("sum_sm", C.c_double), ("sum_dtime", C.c_double),
                ("steps", C.c_int64), ("kernel_ms", C.c_double)]


hip.shq_sfr_on_eeqos.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(SfrParams), _vp, C.c_int64, C.POINTER(CoolingStep), _vp]
hip.shq_starformation.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(SfrFields), _vp, _vp, C.POINTER(SfrParams), _vp, C.c_int64,
                                  C.POINTER(CoolingStep), _vp, C.c_int64, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(SfrResultC)]
hip.shq_sfr_on_eeqos.restype = hip.shq_starformation.restype = C.c_int
_sfr_eval_tail = [C.POINTER(SfrParams), C.c_int, C.c_int64, C.POINTER(SfrArrays), C.POINTER(SfrEvalStep), _vp, _vp, _vp, _vp, _vp, _vp]
hip.shq_sfr_eval.argtypes = [_vp] + _sfr_eval_tail
hip.shq_sfr_eval_host.argtypes = [C.POINTER(CoolingTables)] + _sfr_eval_tail + [C.c_int]
hip.shq_sfr_set_refill.argtypes = [_vp, C.c_int]
hip.shq_sfr_last_kernel.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
for _f in ("shq_sfr_eval", "shq_sfr_eval_host", "shq_sfr_set_refill", "shq_sfr_last_kernel"):
    getattr(hip, _f).restype = C.c_int

hip.shq_treepm_last_fused.argtypes = [_vp, C.POINTER(C.c_int)]
hip.shq_treepm_set_fuse.argtypes = [_vp, C.c_int]
hip.shq_pm_phase_ms.argtypes = [_vp, C.POINTER(C.c_double * 6)]
hip.shq_pm_set_debug.argtypes = [_vp, C.c_int]
hip.shq_pm_set_mesh_scrub.argtypes = [_vp, C.c_int]
hip.shq_pm_mesh_prezeroed.argtypes = [_vp, C.POINTER(C.c_int)]
hip.shq_pm_download_mesh.argtypes = [_vp, C.c_int, _vp]
hip.shq_fft_r2c.argtypes = [_vp, C.c_int, _vp, _vp]
hip.shq_fft_r2c_xyz.argtypes = [_vp, C.c_int, _vp, _vp]
hip.shq_fft_c2r_xyz.argtypes = [_vp, C.c_int, _vp, _vp]
hip.shq_fft_c2r.argtypes = [_vp, C.c_int, _vp, _vp]

host.shqh_last_error.restype = C.c_char_p
GRAVKICK_CB = C.CFUNCTYPE(C.c_double, C.c_int64, C.c_int64, C.c_void_p)
host.shqh_timebinmgr_create.argtypes = [_vp, C.c_int]
host.shqh_timebinmgr_create.restype = _vp
host.shqh_timebinmgr_destroy.argtypes = [_vp]
host.shqh_timebinmgr_destroy.restype = None
host.shqh_timebinmgr_set_gravkick.argtypes = [_vp, GRAVKICK_CB, _vp]
host.shqh_timebinmgr_set_gravkick.restype = None
host.shqh_tbm_ti_from_loga.argtypes = [_vp, C.c_double]
host.shqh_tbm_ti_from_loga.restype = C.c_int64
host.shqh_tbm_loga_from_ti.argtypes = [_vp, C.c_int64]
host.shqh_tbm_loga_from_ti.restype = C.c_double
host.shqh_tbm_dti_from_dloga.argtypes = [_vp, C.c_double, C.c_int64]
host.shqh_tbm_dti_from_dloga.restype = C.c_int64
host.shqh_tbm_dloga_from_dti.argtypes = [_vp, C.c_int64, C.c_int64]
host.shqh_tbm_dloga_from_dti.restype = C.c_double
host.shqh_tbm_get_dloga_for_bin.argtypes = [_vp, C.c_int, C.c_int64]
host.shqh_tbm_get_dloga_for_bin.restype = C.c_double
host.shqh_tbm_find_next_ti_sync.argtypes = [_vp, C.c_int64]
host.shqh_tbm_find_next_ti_sync.restype = C.c_int64
host.shqh_tbm_timeline_at.argtypes = [_vp, C.c_int64, C.POINTER(Timeline)]
host.shqh_tbm_timeline_at.restype = None
host.shqh_round_down_power_of_two.argtypes = [C.c_int64]
host.shqh_round_down_power_of_two.restype = C.c_int64
host.shqh_get_timestep_bin.argtypes = [C.c_int64]
host.shqh_is_timebin_active.argtypes = [C.c_int, C.c_int64]
host.shqh_set_timestep_params.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
host.shqh_set_timestep_params.restype = None
host.shqh_find_timesteps.argtypes = [_vp, C.c_int, C.c_int64, C.POINTER(DriftKickTimes), _vp, C.c_double, C.c_int, C.POINTER(HostCosmo), C.c_double,
                                     C.c_int, C.POINTER(C.c_int)]
host.shqh_find_hydro_timesteps.argtypes = [_vp, C.c_int, C.c_int64, C.POINTER(DriftKickTimes), _vp, C.c_double, C.POINTER(HostCosmo), C.c_int,
                                           C.POINTER(C.c_int)]
host.shqh_hierarchical_gravity_and_timesteps.argtypes = [_vp, C.c_int, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int,
                                                         C.POINTER(DriftKickTimes), _vp, C.c_double, C.c_int, C.c_int, C.POINTER(HostCosmo), C.c_int,
                                                         C.POINTER(C.c_int64)]
host.shqh_partmanager_create.argtypes = [_vp, C.c_int64, C.c_double]
host.shqh_partmanager_create.restype = _vp
host.shqh_partmanager_free.argtypes = [_vp]
host.shqh_partmanager_free.restype = None
host.shqh_force_tree_rebuild_mask.argtypes = [_vp, C.c_int, _vp, C.c_int64, C.c_int]
host.shqh_force_tree_rebuild_mask.restype = _vp
host.shqh_force_tree_free.argtypes = [_vp]
host.shqh_force_tree_free.restype = None
host.shqh_tree_info.argtypes = [_vp, C.POINTER(C.c_int64 * 5)]
host.shqh_tree_info.restype = None
host.shqh_tree_nodes.argtypes = [_vp]
host.shqh_tree_nodes.restype = _vp
host.shqh_tree_father.argtypes = [_vp]
host.shqh_tree_father.restype = _vp
host.shqh_tree_view.argtypes = [_vp, C.POINTER(TreeView)]
host.shqh_tree_view.restype = None
host.shqh_part_view.argtypes = [_vp, C.POINTER(PartView)]
host.shqh_part_view.restype = None
host.shqh_set_kernel_table.argtypes = [_vp]
host.shqh_set_gravshort_treepar.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int]
host.shqh_set_gravshort_treepar.restype = None
host.shqh_gravshort_set_softenings.argtypes = [C.c_double]
host.shqh_gravshort_set_softenings.restype = None
host.shqh_FORCE_SOFTENING.restype = C.c_double
host.shqh_make_grav_params.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(GravParams)]
host.shqh_grav_short_tree.argtypes = [_vp, _vp, _vp, C.c_double, C.c_int, C.c_double, _vp, C.c_int64, _vp,
                                      C.c_double, C.c_int, C.c_int, C.POINTER(WalkStats)]
host.shqh_gravpm_force.argtypes = [_vp, _vp, C.c_double, C.c_int, C.c_double, C.c_int]
# int analysis(userdata, nbins, kk, power, nmodes, Norm, Nmesh, table): gravity.hpp, gravpm_analysis_fn
GRAVPM_ANALYSIS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_double,
                                 C.c_int, C.POINTER(C.c_double))
host.shqh_gravpm_force_hook.argtypes = [_vp, _vp, C.c_double, C.c_int, C.c_double, C.c_int, GRAVPM_ANALYSIS_FN, C.c_void_p, C.c_int]
host.shqh_synth_positions.argtypes = [C.c_int, C.c_int64, C.c_uint64, C.c_double, _vp]
host.shqh_synth_positions.restype = None
host.shqh_synth_positions_range.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_double, _vp]
host.shqh_synth_positions_range.restype = None
host.shqh_morton_order.argtypes = [_vp, C.c_int64, C.c_double, _vp]
host.shqh_morton_order.restype = None
host.shqh_hilbert_order.argtypes = [_vp, C.c_int64, C.c_double, _vp]
host.shqh_hilbert_order.restype = None


def check(rc, where="shq"):
    if rc != 0:
        msg = hip.shq_last_error().decode() or host.shqh_last_error().decode()
        raise ShqError(f"{where} failed with status {rc}: {msg}")


def check_host(rc, where="shqh"):
    if rc != 0:
        msg = host.shqh_last_error().decode() or hip.shq_last_error().decode()
        raise ShqError(f"{where} failed with status {rc}: {msg}")


def ptr(a):
    """void* of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def load_kernel_table():
    tab = np.fromfile(os.path.join(DATADIR, "shortrange_force_kernels.f64"), dtype="<f8").reshape(NGRAVTAB, 5)
    return np.ascontiguousarray(tab)


_KERNELS = load_kernel_table()
host.shqh_set_kernel_table(ptr(_KERNELS))

# ---- SPH host-mirror prototypes --------------------------------------------------------------
hip.shq_density.argtypes = [_vp, C.POINTER(TreeView), _vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhView),
                            _vp, C.c_int64, C.POINTER(DensityParams), _vp, _vp, C.POINTER(SphStats)]
_i64p = C.POINTER(C.c_int64)
hip.shq_density_open.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhView), _vp, C.c_int64,
                                 C.POINTER(DensityParams), C.c_int, _i64p]
hip.shq_density_ev_primary.argtypes = [_vp]
hip.shq_density_ev_secondary.argtypes = [_vp, C.POINTER(DensityParams), _vp, C.c_int64, _vp, _i64p]
hip.shq_density_ev_reduce.argtypes = [_vp, _vp, _vp, C.c_int64]
hip.shq_density_ev_postprocess.argtypes = [_vp, _i64p]
hip.shq_density_close.argtypes = [_vp, _vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhView), _vp, _vp, C.POINTER(SphStats)]
hip.shq_hydro_open.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), _vp, C.c_int64, C.POINTER(HydroParams),
                               _vp, _i64p]
hip.shq_hydro_ev_primary.argtypes = [_vp]
hip.shq_hydro_ev_secondary.argtypes = [_vp, C.POINTER(HydroParams), _vp, C.c_int64, _vp, _i64p]
hip.shq_hydro_ev_reduce.argtypes = [_vp, _vp, _vp, C.c_int64]
hip.shq_hydro_ev_postprocess.argtypes = [_vp]
hip.shq_hydro_close.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(SphStats)]
hip.shq_sph_exports.argtypes = [_vp, _vp, _vp, C.c_int64, _i64p]
hip.shq_sph_fill_queries.argtypes = [_vp, _vp, C.c_int64, _vp]
for _f in ("shq_density_open", "shq_density_ev_primary", "shq_density_ev_secondary", "shq_density_ev_reduce", "shq_density_ev_postprocess",
           "shq_density_close", "shq_hydro_open", "shq_hydro_ev_primary", "shq_hydro_ev_secondary", "shq_hydro_ev_reduce",
           "shq_hydro_ev_postprocess", "shq_hydro_close", "shq_sph_exports", "shq_sph_fill_queries"):
    getattr(hip, _f).restype = C.c_int
hip.shq_stellar_density.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), _vp, C.c_int64,
                                    C.POINTER(StellarParams), _vp, C.POINTER(SphStats)]
hip.shq_stellar_density.restype = C.c_int
hip.shq_bh_veldisp.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), _vp, C.c_int64, C.POINTER(KickFactors), _vp, _vp, _vp, _vp]
hip.shq_bh_veldisp.restype = C.c_int
hip.shq_wind_veldisp.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), _vp, C.c_int64, C.POINTER(KickFactors), C.c_double, C.c_double,
                                 _vp, C.POINTER(SphStats)]
hip.shq_wind_veldisp.restype = C.c_int
class BhDynFricOut(C.Structure):
    _fields_ = [("MinPot", _vp), ("MinPotPos", _vp), ("MinPotVel", _vp), ("updated", _vp), ("DF_SurroundingDensity", _vp),
                ("DF_SurroundingVel", _vp), ("DF_SurroundingRmsVel", _vp)]


hip.shq_bh_dynfric.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), _vp, C.c_int64, C.POINTER(KickFactors), C.c_int, C.c_int, C.c_int,
                               C.POINTER(BhDynFricOut)]
hip.shq_bh_dynfric.restype = C.c_int
hip.shq_hydro_force.argtypes = [_vp, C.POINTER(TreeView), C.POINTER(PartView), C.POINTER(SphView), _vp, C.c_int64,
                                C.POINTER(HydroParams), _vp, C.POINTER(SphStats)]
host.shqh_set_densitypar.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]
host.shqh_set_densitypar.restype = None
host.shqh_GetNumNgb.restype = C.c_double
host.shqh_set_hydropar.argtypes = [C.c_int, C.c_double, C.c_double]
host.shqh_set_hydropar.restype = None
host.shqh_set_init_hsml.argtypes = [_vp, C.c_double, _vp]
host.shqh_force_tree_update_hmax.argtypes = [_vp, _vp]
host.shqh_force_tree_update_hmax.restype = None
host.shqh_density.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, C.c_int, C.c_int, C.c_int,
                              C.POINTER(KickFactors), _vp, _vp, C.c_int, C.POINTER(SphStats)]
host.shqh_hydro_force.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.c_double, C.c_double, _vp,
                                  C.POINTER(KickFactors), _vp, C.c_int, C.POINTER(SphStats)]

# ---- multi-GPU slab entry points -------------------------------------------------------------
hip.shq_particles_set_device.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int]
SET_KEEP_TREE, SET_CARRY_LOCAL = 1, 2              # SHQ_SET_KEEP_TREE, SHQ_SET_CARRY_LOCAL: that call's flags
hip.shq_pm_slab_deposit.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, _vp]
hip.shq_pm_slab_green.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, _vp]
hip.shq_pm_slab_readout.argtypes = [_vp, C.POINTER(PMParams), C.c_int, C.c_int, _vp]
hip.shq_pm_get_deposit_log2scale.argtypes = [_vp]
hip.shq_pm_set_deposit_log2scale.argtypes = [_vp, C.c_int]

# ---- snapshot blocks (csrc/snapshot.hip) ------------------------------------------------------
IO_SELECT_ALL, IO_SELECT_FOF = 0, 1
IO_ORDER_INDEX, IO_ORDER_GRNR = 0, 1
IO_SRC_BASE, IO_SRC_SLOT = 0, 1
IO_F64, IO_F32, IO_I64, IO_U64, IO_I32, IO_U32, IO_I8, IO_U8, IO_BITS = range(9)
IO_COPY, IO_POSITION, IO_SCALE, IO_INTERNAL_ENERGY = range(4)
IO_TYPE_OF_DTYPE = {"f8": IO_F64, "f4": IO_F32, "i8": IO_I64, "u8": IO_U64, "i4": IO_I32, "u4": IO_U32, "i1": IO_I8, "u1": IO_U8}


class IoLayout(C.Structure):
    """shq_io_layout"""
    _fields_ = [("part_elsize", C.c_size_t), ("off_flags", C.c_size_t), ("off_type", C.c_size_t), ("off_pi", C.c_size_t), ("off_grnr", C.c_size_t),
                ("slot_elsize", C.c_size_t * 6)]


class IoBlock(C.Structure):
    """shq_io_block"""
    _fields_ = [("source", C.c_int32), ("kind", C.c_int32), ("field_type", C.c_int32), ("col_type", C.c_int32), ("items", C.c_int32), ("bit_shift", C.c_int32),
                ("bit_width", C.c_int32), ("pad_", C.c_int32), ("offset", C.c_uint64), ("offset2", C.c_uint64)]


class IoConv(C.Structure):
    """shq_io_conv"""
    _fields_ = [("fac", C.c_double), ("atime", C.c_double), ("BoxSize", C.c_double), ("CurrentParticleOffset", C.c_double * 3)]


class IoIonResult(C.Structure):
    """shq_io_ion_result"""
    _fields_ = [("n_status", C.c_int64 * 4), ("n_listed", C.c_int64), ("steps", C.c_int64), ("kernel_ms", C.c_double)]


hip.shq_io_select.argtypes = [_vp, C.POINTER(IoLayout), _vp, C.c_int64, C.c_int, C.c_int, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.shq_io_gather.argtypes = [_vp, C.POINTER(IoLayout), _vp, C.c_int64, _vp, C.POINTER(C.c_int64), C.c_int, _vp, C.c_int64, _vp, C.c_int, C.POINTER(IoConv), _vp]
hip.shq_io_scatter.argtypes = [_vp, C.POINTER(IoLayout), _vp, C.c_int64, _vp, C.POINTER(C.c_int64), C.c_int, C.c_int64, _vp, C.c_int, C.POINTER(IoConv), _vp]
hip.shq_io_ion_fractions.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(SfrFields), C.POINTER(SfrParams), C.POINTER(CoolingStep), _vp, C.c_int64,
                                     C.c_int, _vp, _vp, _vp, C.c_int64, C.POINTER(IoIonResult)]
for _f in ("shq_io_select", "shq_io_gather", "shq_io_scatter", "shq_io_ion_fractions"):
    getattr(hip, _f).restype = C.c_int

# ---- light-cone crossings (csrc/lightcone.hip) ------------------------------------------------
LIGHTCONE_MAXREPLICA = 1000
LIGHTCONE_CONSISTENT, LIGHTCONE_AS_WRITTEN = 0, 1
ERR_INVALID, ERR_NOMEM = 1, 3                      # SHQ_ERR_INVALID, SHQ_ERR_NOMEM


class LightconeParams(C.Structure):
    """shq_lightcone_params"""
    _fields_ = [("zmin", C.c_double), ("zmax", C.c_double), ("ReferenceRedshift", C.c_double), ("BoxBoost", C.c_int32), ("pad_", C.c_int32)]


class LightconeTable(C.Structure):
    """shq_lightcone_table"""
    _fields_ = [("tab_loga", _vp), ("tab_Dc", _vp), ("nentry", C.c_int32), ("pad_", C.c_int32), ("dloga", C.c_double)]


class LightconeState(C.Structure):
    """shq_lightcone_state"""
    _fields_ = [("HorizonDistance", C.c_double), ("HorizonDistance2", C.c_double), ("HorizonDistancePrev", C.c_double), ("HorizonDistance2Prev", C.c_double),
                ("HorizonDistanceRef", C.c_double), ("SampleFraction", C.c_double), ("Nreplica", C.c_int32), ("pad_", C.c_int32),
                ("Reps", (C.c_double * 3) * LIGHTCONE_MAXREPLICA)]


class LightconeLayout(C.Structure):
    """shq_lightcone_layout"""
    _fields_ = [("part_elsize", C.c_size_t), ("off_type", C.c_size_t), ("off_pos", C.c_size_t), ("off_vel", C.c_size_t), ("off_id", C.c_size_t)]


assert C.sizeof(LightconeState) == 56 + 24 * LIGHTCONE_MAXREPLICA
hip.shq_lightcone_horizon.argtypes = [C.POINTER(LightconeTable), C.c_double, C.POINTER(C.c_double)]
hip.shq_lightcone_init.argtypes = [C.POINTER(LightconeTable), C.POINTER(LightconeParams), C.POINTER(LightconeState)]
hip.shq_lightcone_set_time.argtypes = [C.POINTER(LightconeTable), C.POINTER(LightconeParams), C.c_double, C.c_double, C.POINTER(LightconeState)]
hip.shq_lightcone_compute.argtypes = [_vp, C.POINTER(LightconeLayout), _vp, C.c_int64, C.POINTER(LightconeState), C.c_int, C.c_double, C.POINTER(C.c_double), _vp,
                                      C.c_int64, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
hip.shq_lightcone_phase_ms.argtypes = [_vp, C.POINTER(C.c_double)]
for _f in ("shq_lightcone_horizon", "shq_lightcone_init", "shq_lightcone_set_time", "shq_lightcone_compute", "shq_lightcone_phase_ms"):
    getattr(hip, _f).restype = C.c_int

# ---- run start-up (csrc/startup.hip) -------------------------------------------------------------
STARTUP_OMEGA, STARTUP_POSITIONS, STARTUP_HSML, STARTUP_INIT = 1, 2, 4, 8
STARTUP_ALL = 15


class StartupLayout(C.Structure):
    """shq_startup_layout"""
    _fields_ = [(k, C.c_size_t) for k in (
        "part_elsize", "off_pos", "off_mass", "off_flags", "off_type", "off_pi", "off_hsml", "off_ti_drift",
        "sph_elsize", "sph_off_density", "sph_off_egywtdensity", "sph_off_entropy", "sph_off_dtentropy", "sph_off_maxsignalvel", "sph_off_hydroaccel",
        "sph_off_dhsmlegydensityfactor", "sph_off_divvel", "sph_off_curlvel", "sph_off_sfr", "sph_off_ne", "sph_off_delaytime", "sph_off_metallicity",
        "sph_off_metals", "sph_nmetals", "sph_off_local_j21", "sph_off_zreion",
        "bh_elsize", "bh_off_mass", "bh_off_dfaccel", "bh_off_dragaccel")]


class StartupParams(C.Structure):
    """shq_startup_params"""
    _fields_ = [("BoxSize", C.c_double), ("MassTable", C.c_double * 6), ("MeanSeparation", C.c_double * 6), ("Ti_Current", C.c_int64),
                ("generations", C.c_int32), ("RestartSnapNum", C.c_int32), ("init_reion", C.c_int32), ("pad_", C.c_int32)]


class StartupReport(C.Structure):
    """shq_startup_report"""
    _fields_ = [("mass_type", C.c_double * 6), ("mass_total", C.c_double), ("badmass", C.c_int64), ("noutside", C.c_int64), ("first_outside", C.c_int64),
                ("numzero", C.c_int64), ("lastzero", C.c_int64), ("numprob", C.c_int64), ("lastprob", C.c_int64), ("nbad_delaytime", C.c_int64),
                ("first_bad_delaytime", C.c_int64)]


class StartupSmlParams(C.Structure):
    """shq_startup_sml_params"""
    _fields_ = [("density", DensityParams), ("MeanGasSeparation", C.c_double), ("u_init", C.c_double), ("atime", C.c_double),
                ("DensityIndependentSphOn", C.c_int32), ("pad_", C.c_int32)]


class StartupSmlStats(C.Structure):
    """shq_startup_sml_stats"""
    _fields_ = [("first", SphStats), ("nrounds", C.c_int32), ("nmaxdiff", C.c_int32), ("maxdiff", C.c_double * 100), ("nbad_moments", C.c_int64),
                ("nbad_hsml", C.c_int64)]


_dp = C.POINTER(C.c_double)
hip.shq_startup_mean_separation.argtypes = [_dp, C.c_double, C.POINTER(C.c_int64)]
hip.shq_startup_u_init.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp]
hip.shq_startup_omega.argtypes = [_dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _dp, _dp, C.POINTER(C.c_int)]
hip.shq_startup_meanbar.argtypes = [C.c_double, C.c_double, _dp]
hip.shq_startup_particles.argtypes = [_vp, C.POINTER(StartupLayout), _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(StartupParams), C.c_int,
                                      C.POINTER(StartupReport)]
hip.shq_startup_check_density_entropy.argtypes = [_vp, C.POINTER(StartupLayout), _vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)]
hip.shq_set_init_hsml.argtypes = [_vp, C.c_double, C.c_double, _vp]
hip.shq_init_entropy.argtypes = [_vp, C.c_double, C.c_double, C.c_int]
hip.shq_setup_smoothinglengths.argtypes = [_vp, C.POINTER(PartView), C.POINTER(SphView), C.POINTER(BhView), C.POINTER(StartupSmlParams), C.POINTER(StartupSmlStats)]
for _f in ("shq_startup_mean_separation", "shq_startup_u_init", "shq_startup_omega", "shq_startup_meanbar", "shq_startup_particles",
           "shq_startup_check_density_entropy", "shq_set_init_hsml", "shq_init_entropy", "shq_setup_smoothinglengths"):
    getattr(hip, _f).restype = C.c_int

# ---- run logs (csrc/stats.hip) -------------------------------------------------------------------
BHINFO_SIZE = 436


class StatsLayout(C.Structure):
    """shq_stats_layout"""
    _fields_ = [(k, C.c_size_t) for k in (
        "part_elsize", "off_pos", "off_mass", "off_type", "off_pi", "off_vel", "off_potential",
        "sph_elsize", "sph_off_density", "sph_off_entropy", "sph_off_ne", "sph_off_local_j21", "sph_off_zreion")]


class StatsParams(C.Structure):
    """shq_stats_params"""
    _fields_ = [("Time", C.c_double), ("want_temperature", C.c_int32), ("uvbg_mode", C.c_int32), ("GlobalUVBG", CoolingUVBG),
                ("CurrentParticleOffset", C.c_double * 3), ("J21_coeffs", C.c_double * 6), ("ss_greyopac_factor", C.c_double), ("ss_fbar_factor", C.c_double)]


class StatsSums(C.Structure):
    """shq_stats_sums"""
    _fields_ = [("MassComp", C.c_double * 6), ("EnergyPotComp", C.c_double * 6), ("EnergyKinComp", C.c_double * 6), ("EnergyIntComp", C.c_double * 6),
                ("TemperatureComp", C.c_double * 6), ("MomentumComp", C.c_double * 4 * 6), ("AngMomentumComp", C.c_double * 4 * 6),
                ("CenterOfMassComp", C.c_double * 4 * 6), ("count", C.c_int64 * 6), ("n_bad_type", C.c_int64), ("n_status", C.c_int64 * 4),
                ("n_deferred", C.c_int64), ("kernel_ms", C.c_double)]


class StatsState(C.Structure):
    """shq_stats_state (struct state_of_system)"""
    _fields_ = [("Mass", C.c_double), ("EnergyKin", C.c_double), ("EnergyPot", C.c_double), ("EnergyInt", C.c_double), ("EnergyTot", C.c_double),
                ("Momentum", C.c_double * 4), ("AngMomentum", C.c_double * 4), ("CenterOfMass", C.c_double * 4),
                ("MassComp", C.c_double * 6), ("EnergyKinComp", C.c_double * 6), ("EnergyPotComp", C.c_double * 6), ("EnergyIntComp", C.c_double * 6),
                ("EnergyTotComp", C.c_double * 6), ("TemperatureComp", C.c_double * 6), ("MomentumComp", C.c_double * 4 * 6),
                ("AngMomentumComp", C.c_double * 4 * 6), ("CenterOfMassComp", C.c_double * 4 * 6)]


class BhDetailLayout(C.Structure):
    """shq_bh_detail_layout"""
    _fields_ = [(k, C.c_size_t) for k in (
        "part_elsize", "off_pos", "off_mass", "off_flags", "off_type", "off_pi", "off_vel", "off_fulltreegravaccel", "off_id",
        "bh_elsize", "bh_off_mintimebin", "bh_off_encounter", "bh_off_mass", "bh_off_mdot", "bh_off_density", "bh_off_mtrack", "bh_off_kineticfdbkenergy",
        "bh_off_vdisp", "bh_off_dfaccel", "bh_off_df_surroundingvel", "bh_off_df_surroundingrmsvel", "bh_off_df_surroundingdensity", "bh_off_dragaccel",
        "bh_off_swallowid", "bh_off_minpot", "bh_off_minpotpos", "bh_off_countprogs")]


BH_DETAIL_ARRAYS = ("BH_Entropy", "BH_SurroundingGasVel", "BH_accreted_momentum", "BH_accreted_Mass", "BH_accreted_BHMass", "BH_FeedbackWeightSum", "NumDM",
                    "MgasEnc", "KEflag", "SPH_SwallowID")


class BhDetailArrays(C.Structure):
    """shq_bh_detail_arrays"""
    _fields_ = [(k, _vp) for k in BH_DETAIL_ARRAYS] + [("n_sph_swallowid", C.c_int64), ("CurrentParticleOffset", C.c_double * 3)]


hip.shq_energy_statistics.argtypes = [_vp, C.POINTER(StatsLayout), _vp, C.c_int64, _vp, C.c_int64, C.POINTER(StatsParams), C.POINTER(StatsSums), _vp, C.c_int64]
hip.shq_stats_finish.argtypes = [C.POINTER(StatsSums), C.POINTER(StatsState)]
hip.shq_bh_totals.argtypes = [_vp, _vp, C.c_int64, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64), _dp]
hip.shq_bh_details.argtypes = [_vp, C.POINTER(BhDetailLayout), _vp, C.c_int64, _vp, C.c_int64, C.POINTER(BhDetailArrays), _vp, C.c_int64, C.c_double, _vp]
for _f in ("shq_energy_statistics", "shq_stats_finish", "shq_bh_totals", "shq_bh_details"):
    getattr(hip, _f).restype = C.c_int

# ---- linear-response massive neutrinos (csrc/nulra.hip, csrc/nulra_host.hip) ---------------------
NULRA_COSMO_FN = C.CFUNCTYPE(C.c_double, C.c_double, C.c_int, C.c_void_p)


class NulraParams(C.Structure):
    """shq_nulra_params"""
    _fields_ = [("nk_allocated", C.c_int32), ("hybrid_enabled", C.c_int32), ("TimeTransfer", C.c_double), ("TimeMax", C.c_double),
                ("light", C.c_double), ("delta_nu_prefac", C.c_double), ("Omeganonu", C.c_double), ("OmegaNu1", C.c_double), ("kBtnu", C.c_double),
                ("mnu", C.c_double * 3), ("degeneracy", C.c_double * 3), ("vcrit_by_light", C.c_double), ("nu_crit_time", C.c_double),
                ("nufrac_low", C.c_double * 3), ("BoxSize_in_MPC", C.c_double), ("NPowerTable", C.c_int32), ("pad_", C.c_int32),
                ("logk", _vp), ("T_nu", _vp), ("hubble", NULRA_COSMO_FN), ("omega_nu_nopart", NULRA_COSMO_FN), ("omega_nu_single", NULRA_COSMO_FN),
                ("user", C.c_void_p)]


class NulraState(C.Structure):
    """shq_nulra_state"""
    _fields_ = [("ia", C.c_int32), ("nk", C.c_int32), ("scalefact", _vp), ("delta_tot", _vp), ("delta_nu_init", _vp), ("kvalue", _vp), ("delta_nu_last", _vp)]


class NulraInfo(C.Structure):
    """shq_nulra_info"""
    _fields_ = [("ia", C.c_int32), ("nk", C.c_int32), ("nonzero", C.c_int32), ("namax", C.c_int32), ("kept", C.c_int32), ("nnodes", C.c_int32),
                ("nu_prefac", C.c_double), ("ms", C.c_double * 3), ("callback_s", C.c_double)]


hip.shq_nulra_init.argtypes = [_vp, C.POINTER(NulraParams)]
hip.shq_nulra_free.argtypes = [_vp]
hip.shq_nulra_host_create.argtypes = [C.POINTER(NulraParams), C.POINTER(C.c_void_p)]
hip.shq_nulra_host_destroy.argtypes = [_vp]
hip.shq_nulra_host_destroy.restype = None
for _p in ("shq_nulra_", "shq_nulra_host_"):
    getattr(hip, _p + "step").argtypes = [_vp, C.c_double, C.c_double, _vp, C.c_int]
    getattr(hip, _p + "mode_table").argtypes = [_vp, C.c_int, C.c_int, _vp]
    getattr(hip, _p + "download").argtypes = [_vp, _vp, _vp, C.POINTER(NulraInfo)]
    getattr(hip, _p + "delta_nu").argtypes = [_vp, C.c_double, _vp]
    getattr(hip, _p + "get_state").argtypes = [_vp, C.POINTER(NulraState)]
    getattr(hip, _p + "set_state").argtypes = [_vp, C.POINTER(NulraState)]
    for _f in ("step", "mode_table", "download", "delta_nu", "get_state", "set_state"):
        getattr(hip, _p + _f).restype = C.c_int
for _f in ("shq_nulra_init", "shq_nulra_free", "shq_nulra_host_create"):
    getattr(hip, _f).restype = C.c_int
