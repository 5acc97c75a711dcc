"""ctypes binding of the C ABI declared in include/scema_md.h (libscema_md.so).

This is the only way Python reaches the engine: plain pointers and sizes, no torch types.  The
library is built in-tree by `scema_amd/csrc/Makefile` (`__graft_entry__.build()`); there is no CPU
fallback -- a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# tools/run_asan.sh (CPU tests only): the build whose host layer is compiled with AddressSanitizer + UBSan
# SCEMA_MD_LIB=<file name in this directory>: an A/B build of the library for same-box kernel comparisons (csrc/Makefile: LIBNAME);
# bench.py lists the variable under config.env_overrides
LIB_PATH = os.path.join(_HERE, os.environ.get("SCEMA_MD_LIB") or ("libscema_md_asan.so" if os.environ.get("SCEMA_SANITIZE") == "1" else "libscema_md.so"))

NPART = 8
PARTS = ["lj", "coul", "bond", "angle", "dihedral", "improper", "kspace", "shake"]
QP_NONE = -1  # uint32 max as int32 (stmd_problem.h:126)

# every symbol include/scema_md.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "scema_md_default_params", "scema_md_create", "scema_md_destroy", "scema_md_last_error",
    "scema_md_register_replica", "scema_md_load_replica_file", "scema_md_write_replica_file",
    "scema_md_load_lammps_data", "scema_md_convert_lammps_data",
    "scema_md_probe_lammps_restart", "scema_md_read_lammps_restart_atoms", "scema_md_load_lammps_restart",
    "scema_md_convert_lammps_restart", "scema_md_write_lammps_restart",
    "scema_md_strain_batch", "scema_md_strain", "scema_md_local_stress_device_ptr",
    "scema_md_local_stress_count", "scema_md_local_result_doubles", "scema_md_copy_local_stress", "scema_md_scatter_gathered", "scema_md_settle_update", "scema_md_has_state", "scema_md_get_state",
    "scema_md_set_state", "scema_md_drop_state", "scema_md_save_state_file", "scema_md_load_state_file", "scema_md_save_state_lammps",
    "scema_md_init_material", "scema_md_debug_compute", "scema_md_debug_run", "scema_md_debug_skin_bands", "scema_md_debug_rows", "scema_md_get_profile", "scema_md_env_overrides",
    "scema_md_comm_unique_id", "scema_md_comm_init_rccl", "scema_md_comm_init_host", "scema_md_comm_destroy",
    "scema_md_comm_world", "scema_md_comm_rank", "scema_md_comm_stats", "scema_md_comm_handshakes", "scema_md_state_owner", "scema_md_last_plan",
    "scema_plan_dir_create", "scema_plan_dir_destroy", "scema_plan_update", "scema_md_kspace_setup",
    "scema_md_save_state_dump", "scema_md_replica_natoms", "scema_md_save_replica_file", "scema_md_equilibrate", "scema_md_debug_minimize", "scema_md_debug_run_nh",
    "scema_md_reax_configure", "scema_md_reax_activate", "scema_md_reax_set", "scema_md_reax_concurrency", "scema_md_batch_split", "scema_md_get_concurrency", "scema_md_pppm_plan_count", "scema_md_pppm_tiling", "scema_md_pppm_binning", "scema_md_bonded_grouping","scema_md_pppm_force_layout", "scema_md_pppm_force_strides", "scema_md_pppm_binned_launches", "scema_md_pppm_paths", "scema_md_pppm_tile_shape", "scema_md_unsettled_updates", "scema_md_reax_debug_compute", "scema_md_reax_stats", "scema_md_box_fma_tflops",
    "scema_md_sw_configure", "scema_md_sw_debug_compute", "scema_md_sw_read_params",
    "scema_md_tersoff_configure", "scema_md_tersoff_debug_compute", "scema_md_tersoff_read_params",
    "scema_md_eam_configure", "scema_md_eam_debug_compute", "scema_md_eam_read_setfl",
    "scema_md_tersoff_mod_configure", "scema_md_tersoff_mod_debug_compute", "scema_md_tersoff_mod_read_params",
    "scema_md_tersoff_zbl_configure", "scema_md_tersoff_zbl_debug_compute", "scema_md_tersoff_zbl_read_params",
    "scema_md_vashishta_configure", "scema_md_vashishta_debug_compute", "scema_md_vashishta_read_params",
    "scema_md_adp_configure", "scema_md_adp_debug_compute", "scema_md_adp_read_setfl",
    "scema_md_edip_configure", "scema_md_edip_debug_compute", "scema_md_edip_read_params",
    "scema_md_meam_spline_configure", "scema_md_meam_spline_debug_compute", "scema_md_meam_spline_read_params", "scema_md_meam_spline_eval",
    "scema_md_born_dsf_configure", "scema_md_born_dsf_debug_compute", "scema_md_born_dsf_read_params", "scema_md_born_dsf_eval",
    "scema_md_born_long_configure", "scema_md_born_long_debug_compute", "scema_md_born_long_read_params", "scema_md_born_long_eval",
    "scema_md_born_long_kvectors", "scema_md_born_long_kspace", "scema_md_born_long_last_mesh", "scema_md_born_long_mesh",
    "scema_md_eam_coul_configure", "scema_md_eam_coul_debug_compute", "scema_md_eam_coul_kspace", "scema_md_eam_coul_last_mesh",
    "scema_md_eam_coul_read_params",
]
COMM_ID_BYTES = 128
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
HOST_SEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)
HOST_RECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)


class EquilParams(C.Structure):
    _fields_ = [("nsteps_equil", C.c_int32), ("timestep_length", C.c_double), ("temperature", C.c_double), ("seed", C.c_int64)]


class Params(C.Structure):
    _fields_ = [("cut_lj", C.c_double), ("cut_coul", C.c_double), ("skin", C.c_double), ("neigh_delay", C.c_int32),
                ("kspace_accuracy", C.c_double), ("shake_tol", C.c_double), ("shake_maxiter", C.c_int32),
                ("shake_mass", C.c_double), ("t_period", C.c_double), ("t_chain", C.c_int32), ("device", C.c_int32),
                ("max_batch", C.c_int32), ("profile", C.c_int32), ("kspace_style", C.c_int32)]


_P = C.c_void_p


class System(C.Structure):
    _fields_ = [("natoms", C.c_int32), ("ntypes", C.c_int32), ("type", _P), ("charge", _P), ("mass", _P),
                ("eps", _P), ("sigma", _P),
                ("nbonds", C.c_int32), ("nbondtypes", C.c_int32), ("bond_atoms", _P), ("bond_type", _P), ("bond_coeff", _P),
                ("nangles", C.c_int32), ("nangletypes", C.c_int32), ("angle_atoms", _P), ("angle_type", _P), ("angle_coeff", _P),
                ("ndihedrals", C.c_int32), ("ndihedraltypes", C.c_int32), ("dihedral_atoms", _P), ("dihedral_type", _P),
                ("dihedral_coeff", _P),
                ("nimpropers", C.c_int32), ("nimpropertypes", C.c_int32), ("improper_atoms", _P), ("improper_type", _P),
                ("improper_coeff", _P),
                ("special_lj", C.c_double * 3), ("special_coul", C.c_double * 3), ("box", C.c_double * 9), ("x", _P), ("v", _P)]


class MDSim(C.Structure):
    """Mirror of HMM::MDSim<3> (headers/md_sim.h:15-58)."""
    _fields_ = [("qp_id", C.c_int32), ("most_recent_qp_id", C.c_int32), ("replica", C.c_int32), ("material", C.c_int32),
                ("matid", C.c_char_p), ("time_id", C.c_char_p), ("output_folder", C.c_char_p),
                ("restart_folder", C.c_char_p), ("scripts_folder", C.c_char_p), ("log_file", C.c_char_p),
                ("force_field", C.c_char_p),
                ("strain", C.c_double * 6), ("stiffness", C.c_double * 36),
                ("timestep_length", C.c_double), ("temperature", C.c_double), ("strain_rate", C.c_double),
                ("nsteps_sample", C.c_int32), ("output_homog", C.c_int32), ("checkpoint", C.c_int32),
                ("stress", C.c_double * 6), ("stress_updated", C.c_int32)]


class EqParams(C.Structure):
    """scema_md_eqparams (include/scema_md.h)."""
    _fields_ = [("timestep_length", C.c_double), ("temperature", C.c_double), ("nsteps_sample", C.c_int32),
                ("strain_ampl", C.c_double), ("strain_rate", C.c_double)]


class Profile(C.Structure):
    _fields_ = [("pair_launches", C.c_int64), ("pair_ms", C.c_double), ("pair_alg_bytes", C.c_double),
                ("md_steps", C.c_int64), ("neigh_builds", C.c_int64), ("unique_pairs_per_sim", C.c_double),
                ("evals", C.c_int64), ("list_skin_mean", C.c_double), ("pair_sims", C.c_int64), ("box_flips", C.c_int64),
                ("rx_sweep_launches", C.c_int64), ("rx_sweep_ms", C.c_double), ("rx_sweep_entries", C.c_double), ("rx_sweep_rows", C.c_double), ("rx_sweep_col_bytes", C.c_int64),
                ("pair_union_ms", C.c_double), ("rx_sweep_union_ms", C.c_double), ("rx_sweep_symmetric", C.c_int64),
                ("row_cell_builds", C.c_int64)]


_lib = None


def lib():
    """Load libscema_md.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(make -C scema_amd/csrc); the engine has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.scema_md_last_error.restype = C.c_char_p
        L.scema_md_last_error.argtypes = [_P]
        L.scema_md_local_stress_device_ptr.restype = C.c_void_p
        L.scema_md_local_stress_device_ptr.argtypes = [_P]
        L.scema_md_local_stress_count.argtypes = [_P]
        L.scema_md_destroy.argtypes = [_P]
        L.scema_md_destroy.restype = None
        L.scema_md_comm_destroy.argtypes = [_P]
        L.scema_md_comm_destroy.restype = None
        L.scema_md_comm_world.argtypes = [_P]
        L.scema_md_comm_rank.argtypes = [_P]
        L.scema_plan_dir_create.restype = C.c_void_p
        L.scema_plan_dir_destroy.argtypes = [_P]
        L.scema_plan_dir_destroy.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_params(**kw) -> Params:
    p = Params()
    lib().scema_md_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_system(d: dict):
    """Build a `System` struct from the dict produced by scema_amd.systems.build_pe; returns
    (struct, keepalive list)."""
    a = lambda k, t: np.ascontiguousarray(d[k], dtype=t)
    keep = dict(type=a("type", np.int32), charge=a("charge", np.float64), mass=a("mass", np.float64),
                eps=a("eps", np.float64), sigma=a("sigma", np.float64),
                bonds=a("bonds", np.int32), bond_type=a("bond_type", np.int32), bond_coeff=a("bond_coeff", np.float64),
                angles=a("angles", np.int32), angle_type=a("angle_type", np.int32), angle_coeff=a("angle_coeff", np.float64),
                dihedrals=a("dihedrals", np.int32), dihedral_type=a("dihedral_type", np.int32),
                dihedral_coeff=a("dihedral_coeff", np.float64),
                impropers=a("impropers", np.int32), improper_type=a("improper_type", np.int32),
                improper_coeff=a("improper_coeff", np.float64), x=a("x", np.float64), v=a("v", np.float64))
    s = System()
    s.natoms = int(d["natoms"]); s.ntypes = int(d["ntypes"])
    s.type = _p(keep["type"]); s.charge = _p(keep["charge"]); s.mass = _p(keep["mass"])
    s.eps = _p(keep["eps"]); s.sigma = _p(keep["sigma"])
    s.nbonds = len(keep["bond_type"]); s.nbondtypes = len(keep["bond_coeff"])
    s.bond_atoms = _p(keep["bonds"]); s.bond_type = _p(keep["bond_type"]); s.bond_coeff = _p(keep["bond_coeff"])
    s.nangles = len(keep["angle_type"]); s.nangletypes = len(keep["angle_coeff"])
    s.angle_atoms = _p(keep["angles"]); s.angle_type = _p(keep["angle_type"]); s.angle_coeff = _p(keep["angle_coeff"])
    s.ndihedrals = len(keep["dihedral_type"]); s.ndihedraltypes = len(keep["dihedral_coeff"])
    s.dihedral_atoms = _p(keep["dihedrals"]); s.dihedral_type = _p(keep["dihedral_type"])
    s.dihedral_coeff = _p(keep["dihedral_coeff"])
    s.nimpropers = len(keep["improper_type"]); s.nimpropertypes = len(keep["improper_coeff"])
    s.improper_atoms = _p(keep["impropers"]); s.improper_type = _p(keep["improper_type"])
    s.improper_coeff = _p(keep["improper_coeff"])
    s.special_lj[:] = list(np.asarray(d["special_lj"], float))
    s.special_coul[:] = list(np.asarray(d["special_coul"], float))
    s.box[:] = list(np.asarray(d["box"], float))
    s.x = _p(keep["x"]); s.v = _p(keep["v"])
    return s, keep


class RestartInfo(C.Structure):
    """scema_lammps_restart_info (include/scema_md.h)."""
    _fields_ = [("version", C.c_char * 32), ("units", C.c_char * 16), ("atom_style", C.c_char * 32), ("pair_style", C.c_char * 64),
                ("natoms", C.c_int64), ("ntimestep", C.c_int64), ("nbonds", C.c_int64), ("nangles", C.c_int64),
                ("ndihedrals", C.c_int64), ("nimpropers", C.c_int64),
                ("ntypes", C.c_int32), ("nbondtypes", C.c_int32), ("nangletypes", C.c_int32), ("ndihedraltypes", C.c_int32),
                ("nimpropertypes", C.c_int32), ("triclinic", C.c_int32), ("nprocs", C.c_int32), ("reserved", C.c_int32),
                ("box", C.c_double * 9), ("timestep", C.c_double), ("special_lj", C.c_double * 3), ("special_coul", C.c_double * 3),
                ("cut_lj", C.c_double), ("cut_coul", C.c_double), ("mass", C.c_double * 16), ("error", C.c_char * 160)]


def probe_lammps_restart(path: str) -> RestartInfo:
    info = RestartInfo()
    rc = lib().scema_md_probe_lammps_restart(path.encode(), C.byref(info))
    if rc != 0:
        raise IOError(f"{path}: rc={rc}: {info.error.decode()}")
    return info


def read_lammps_restart_atoms(path: str, natoms: int) -> dict:
    tag = np.zeros(natoms, np.int64); typ = np.zeros(natoms, np.int32); img = np.zeros((natoms, 3), np.int32)
    x = np.zeros((natoms, 3)); v = np.zeros((natoms, 3))
    rc = lib().scema_md_read_lammps_restart_atoms(path.encode(), C.c_int64(natoms), _p(tag), _p(typ), _p(img), _p(x), _p(v))
    if rc != 0:
        raise IOError(f"{path}: rc={rc}")
    return dict(tag=tag, type=typ, image=img, x=x, v=v)


def write_lammps_restart(path: str, sysd: dict, cut_lj: float, cut_coul: float, timestep: float = 2.0, ntimestep: int = 0):
    s, keep = make_system(sysd)
    rc = lib().scema_md_write_lammps_restart(path.encode(), C.byref(s), C.c_double(cut_lj), C.c_double(cut_coul),
                                             C.c_double(timestep), C.c_int64(ntimestep))
    if rc != 0:
        raise IOError(f"cannot write {path} (rc={rc})")


REAX_PARTS = ["bond", "lp", "over", "under", "angle", "pen", "coa", "tors", "conj", "hb", "vdw", "coul", "pol"]


def reax_system(symbols, x, box, v=None, elements=("H", "C", "N", "O"), masses=(1.008, 12.011, 14.007, 15.999)) -> dict:
    """System dict of a ReaxFF replica (atom_style charge, lammps_scripts_reax/in.set.lammps:17): LAMMPS type k+1 = elements[k],
    no bonded topology; charges are equilibrated by the engine every step."""
    n = len(symbols)
    nt = len(elements)
    z2 = np.zeros((0, 2))
    return dict(natoms=n, ntypes=nt, type=np.array([elements.index(s) for s in symbols], np.int32), charge=np.zeros(n), mass=np.array(masses, float),
                eps=np.zeros((nt, nt)), sigma=np.ones((nt, nt)), bonds=np.zeros((0, 2), np.int32), bond_type=np.zeros(0, np.int32), bond_coeff=z2,
                angles=np.zeros((0, 3), np.int32), angle_type=np.zeros(0, np.int32), angle_coeff=z2, dihedrals=np.zeros((0, 4), np.int32),
                dihedral_type=np.zeros(0, np.int32), dihedral_coeff=np.zeros((0, 4)), impropers=np.zeros((0, 4), np.int32),
                improper_type=np.zeros(0, np.int32), improper_coeff=z2, special_lj=np.zeros(3), special_coul=np.zeros(3),
                box=np.asarray(box, float), x=np.asarray(x, float), v=np.zeros((n, 3)) if v is None else np.asarray(v, float))


class EngineError(RuntimeError):
    pass


class Engine:
    """Thin owner of a `scema_md_engine*`."""

    def __init__(self, params: Params | None = None, **kw):
        L = lib()
        self.params = params if params is not None else default_params(**kw)
        self.h = C.c_void_p()
        rc = L.scema_md_create(C.byref(self.params), C.byref(self.h))
        if rc != 0:
            raise EngineError(f"scema_md_create failed (rc={rc}): no usable HIP device; the engine has no CPU fallback")
        self._natoms = {}

    def close(self):
        if self.h:
            lib().scema_md_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(f"rc={rc}: {lib().scema_md_last_error(self.h).decode()}")

    def register_replica(self, matid: str, replica: int, sysd: dict):
        s, keep = make_system(sysd)
        self._chk(lib().scema_md_register_replica(self.h, matid.encode(), C.c_int32(replica), C.byref(s)))
        self._natoms[(matid, replica)] = int(sysd["natoms"])

    def load_replica_file(self, matid: str, replica: int, path: str, natoms: int | None = None):
        self._chk(lib().scema_md_load_replica_file(self.h, matid.encode(), C.c_int32(replica), path.encode()))
        if natoms is not None:
            self._natoms[(matid, replica)] = natoms

    def load_lammps_data(self, matid: str, replica: int, path: str, natoms: int, special_lj=None, special_coul=None):
        slj = None if special_lj is None else np.ascontiguousarray(special_lj, np.float64)
        sc = None if special_coul is None else np.ascontiguousarray(special_coul, np.float64)
        self._chk(lib().scema_md_load_lammps_data(self.h, matid.encode(), C.c_int32(replica), path.encode(), _p(slj), _p(sc)))
        self._natoms[(matid, replica)] = natoms

    def load_lammps_restart(self, matid: str, replica: int, path: str, natoms: int):
        self._chk(lib().scema_md_load_lammps_restart(self.h, matid.encode(), C.c_int32(replica), path.encode()))
        self._natoms[(matid, replica)] = natoms

    def strain_batch(self, sims, hooke: bool = False, rank: int = 0, world: int = 1):
        arr = (MDSim * len(sims))(*sims) if not isinstance(sims, C.Array) else sims
        self._chk(lib().scema_md_strain_batch(self.h, arr, C.c_int32(len(arr)), C.c_int32(1 if hooke else 0),
                                              C.c_int32(rank), C.c_int32(world)))
        return arr

    def local_stress_ptr(self):
        return lib().scema_md_local_stress_device_ptr(self.h), lib().scema_md_local_stress_count(self.h)

    def local_result_doubles(self) -> int:
        """doubles in the result buffer of the last strain_batch: 6*max(cap,1) stresses + status word + plan hash"""
        return int(lib().scema_md_local_result_doubles(self.h))

    def copy_local_stress(self, dst_ptr: int, on_device: bool):
        self._chk(lib().scema_md_copy_local_stress(self.h, C.c_void_p(dst_ptr), C.c_int32(1 if on_device else 0)))

    def scatter_gathered(self, gathered: np.ndarray, arr):
        g = np.ascontiguousarray(gathered, np.float64)
        self._chk(lib().scema_md_scatter_gathered(self.h, _p(g), arr, C.c_int32(len(arr))))

    def last_plan(self, n: int):
        """(owner[n], pos[n], cap) of the last strain_batch (host/sim_plan.h)."""
        owner = np.zeros(n, np.int32); pos = np.zeros(n, np.int32); cap = C.c_int32(0)
        self._chk(lib().scema_md_last_plan(self.h, C.c_int32(n), _p(owner), _p(pos), C.byref(cap)))
        return owner, pos, cap.value

    # ---- communicator: one process per GPU ----
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = lib().scema_md_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(f"scema_md_comm_unique_id failed (rc={rc})")
        return buf.raw

    def comm_init_rccl(self, uid: bytes, rank: int, world: int):
        assert len(uid) == COMM_ID_BYTES
        self._chk(lib().scema_md_comm_init_rccl(self.h, C.c_char_p(uid), C.c_int32(rank), C.c_int32(world)))

    def comm_init_host(self, rank: int, world: int, allgather, send=None, recv=None):
        """Host transport: allgather(send: bytes) -> bytes of all ranks; send(data: bytes, dst); recv(nbytes, src) -> bytes."""
        def _ag(ctx, sp, rp, nbytes):
            try:
                out = allgather(C.string_at(sp, nbytes))
                C.memmove(rp, out, nbytes * world)
                return 0
            except Exception:
                return 1

        def _send(ctx, p, nbytes, dst):
            try:
                send(C.string_at(p, nbytes), dst)
                return 0
            except Exception:
                return 1

        def _recv(ctx, p, nbytes, src):
            try:
                C.memmove(p, recv(nbytes, src), nbytes)
                return 0
            except Exception:
                return 1

        self._cb = (HOST_ALLGATHER_FN(_ag), HOST_SEND_FN(_send) if send else C.cast(None, HOST_SEND_FN),
                    HOST_RECV_FN(_recv) if recv else C.cast(None, HOST_RECV_FN))
        self._chk(lib().scema_md_comm_init_host(self.h, C.c_int32(rank), C.c_int32(world), self._cb[0], self._cb[1], self._cb[2], None))

    def comm_destroy(self):
        lib().scema_md_comm_destroy(self.h)

    def comm_stats(self) -> dict:
        a = C.c_int64(0); m = C.c_int64(0)
        self._chk(lib().scema_md_comm_stats(self.h, C.byref(a), C.byref(m)))
        lib().scema_md_comm_handshakes.restype = C.c_int64
        lib().scema_md_comm_handshakes.argtypes = [_P]
        return dict(allgathers=a.value, migrations=m.value, handshakes=int(lib().scema_md_comm_handshakes(self.h)))

    def state_owner(self, qp, matid, replica) -> int:
        return int(lib().scema_md_state_owner(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica)))

    def has_state(self, qp, matid, replica) -> bool:
        return bool(lib().scema_md_has_state(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica)))

    def natoms(self, matid, replica) -> int:
        """atoms of a registered replica (also one the library registered itself, e.g. from a file)"""
        if (matid, replica) not in self._natoms:
            n = int(lib().scema_md_replica_natoms(self.h, matid.encode(), C.c_int32(replica)))
            if n <= 0:
                raise EngineError(f"replica {matid}_{replica} is not registered")
            self._natoms[(matid, replica)] = n
        return self._natoms[(matid, replica)]

    def get_state(self, qp, matid, replica):
        n = self.natoms(matid, replica)
        box = np.zeros(9); x = np.zeros((n, 3)); v = np.zeros((n, 3))
        self._chk(lib().scema_md_get_state(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(box), _p(x), _p(v)))
        return box, x, v

    def set_state(self, qp, matid, replica, box, x, v):
        box = np.ascontiguousarray(box, np.float64); x = np.ascontiguousarray(x, np.float64); v = np.ascontiguousarray(v, np.float64)
        self._chk(lib().scema_md_set_state(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(box), _p(x), _p(v)))

    def drop_state(self, qp, matid, replica):
        self._chk(lib().scema_md_drop_state(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica)))

    def save_state_file(self, qp, matid, replica, path):
        self._chk(lib().scema_md_save_state_file(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), path.encode()))

    def save_state_lammps(self, qp, matid, replica, path, timestep=2.0, ntimestep=0):
        self._chk(lib().scema_md_save_state_lammps(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), path.encode(),
                                                   C.c_double(timestep), C.c_int64(ntimestep)))

    def save_state_dump(self, qp, matid, replica, path, ntimestep=0, precise=True):
        self._chk(lib().scema_md_save_state_dump(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), path.encode(), C.c_int64(ntimestep),
                                                 C.c_int32(1 if precise else 0)))

    def load_state_file(self, qp, matid, replica, path):
        self._chk(lib().scema_md_load_state_file(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), path.encode()))

    def debug_compute(self, matid, replica, qp=QP_NONE, use_shake=False):
        n = self._natoms[(matid, replica)]
        f = np.zeros((n, 3)); e = np.zeros(NPART); w = np.zeros((NPART, 6)); info = np.zeros(8)
        self._chk(lib().scema_md_debug_compute(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica),
                                               C.c_int32(1 if use_shake else 0), _p(f), _p(e), _p(w), _p(info)))
        return f, e, w, dict(g_ewald=info[0], nk=int(info[1]), npairs=info[2], tdof=info[3], t_current=info[4],
                             maxneigh_seen=int(info[5]), maxneigh=int(info[6]), nclus=int(info[7]))

    def debug_run(self, matid, replica, nsteps, dt, temperature, qp=QP_NONE, nvt=True, use_shake=True, rates=None, sample=False):
        r = None if rates is None else np.ascontiguousarray(rates, np.float64)
        pavg = np.zeros(6) if sample else None
        self._chk(lib().scema_md_debug_run(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), C.c_int32(nsteps),
                                           C.c_double(dt), C.c_double(temperature), C.c_int32(1 if nvt else 0),
                                           C.c_int32(1 if use_shake else 0), _p(r), _p(pavg)))
        return pavg

    def debug_skin_bands(self, pos=0):
        """Skin bands of the pair rows of the replica at position `pos` of the last run, as its next pair launch would walk them:
        dict(K, listed[K], walked[K], rows, rows_open, rows_all_open) (skin entries per band; rows with skin entries)."""
        out = np.zeros(64, np.uint64)
        self._chk(lib().scema_md_debug_skin_bands(self.h, C.c_int32(pos), out.ctypes.data_as(C.c_void_p), C.c_int32(out.size)))
        k = int(out[0])
        return dict(K=k, listed=[int(v) for v in out[1:1 + k]], walked=[int(v) for v in out[1 + k:1 + 2 * k]],
                    rows=int(out[1 + 2 * k]), rows_open=int(out[2 + 2 * k]), rows_all_open=int(out[3 + 2 * k]))

    def debug_rows(self, pos=0, rows=True):
        """Neighbour rows of the replica at position `pos` of the last run or static evaluation of a row potential: dict(n, cap, cells
        (1: built through cells), ncell[3], and with `rows` cnt[n] and rows[n, cap]: atom | image code << 24, ascending by atom)."""
        info = np.zeros(6, np.int32)
        f = lib().scema_md_debug_rows
        f.argtypes = [_P, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._chk(f(self.h, pos, None, None, 0, info.ctypes.data))
        out = dict(n=int(info[0]), cap=int(info[1]), cells=int(info[2]), ncell=[int(v) for v in info[3:6]])
        if rows:
            cnt = np.zeros(out["n"], np.int32)
            tab = np.zeros((out["n"], out["cap"]), np.int32)
            self._chk(f(self.h, pos, cnt.ctypes.data, tab.ctypes.data, tab.size, info.ctypes.data))
            out.update(cnt=cnt, rows=tab)
        return out

    def init_material(self, matid, replica, dt=2.0, temperature=300.0, nss=100, strain_ampl=0.005, strain_rate=1e-4):
        """EQMDProblem::lammps_equilibration for an equilibrated replica (init_material_problem.h:196-300): returns
        (length[3], stress[6] Pa file order 00,01,02,11,12,22, stiff[6,6] Pa file order)."""
        p = EqParams(dt, temperature, nss, strain_ampl, strain_rate)
        length, stress, stiff = np.zeros(3), np.zeros(6), np.zeros(36)
        self._chk(lib().scema_md_init_material(self.h, matid.encode(), C.c_int32(replica), C.byref(p), _p(length), _p(stress), _p(stiff)))
        return length, stress, stiff.reshape(6, 6)

    # ---- ReaxFF replicas (force_field "reax") ----
    def reax_configure(self, ffield: str, elements=("H", "C", "N", "O"), qeq_tol: float = 1e-6, skin: float = -1.0):
        """pair_coeff * * <ffield> H C N O + fix qeq/reax 1 0.0 10.0 <qeq_tol> (lammps_scripts_reax/in.strain.lammps:10-12)"""
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self._chk(lib().scema_md_reax_configure(self.h, ffield.encode(), arr, C.c_int32(len(elements)), C.c_double(qeq_tol), C.c_double(skin)))

    def reax_activate(self, on: bool = True):
        self._chk(lib().scema_md_reax_activate(self.h, C.c_int32(1 if on else 0)))

    def reax_set(self, exact_gradient: int = -1, terms: int = -1, qeq_maxiter: int = -1):
        self._chk(lib().scema_md_reax_set(self.h, C.c_int32(exact_gradient), C.c_int32(terms), C.c_int32(qeq_maxiter)))

    def reax_concurrency(self, halves: int = -1, overlap: int = -1):
        """how a ReaxFF batch is issued (two half batches on two streams; bond-order chain next to the charge chain): 1 / 0, -1 leaves it"""
        self._chk(lib().scema_md_reax_concurrency(self.h, C.c_int32(halves), C.c_int32(overlap)))

    def unsettled_updates(self) -> int:
        lib().scema_md_unsettled_updates.restype = C.c_int64
        return int(lib().scema_md_unsettled_updates(self.h))

    def batch_split(self, on: int = -1):
        self._chk(lib().scema_md_batch_split(self.h, C.c_int32(on)))

    def pppm_plan_count(self) -> int:
        """batched hipFFT plans the engine holds (one per mesh size, batch count and stream)"""
        lib().scema_md_pppm_plan_count.restype = C.c_int
        return int(lib().scema_md_pppm_plan_count(self.h))

    def pppm_tiling(self, mode: int = -1, lds_bytes: int = -1):
        """tiled PPPM kernels for meshes beyond the LDS (1, default) or the kernels without LDS (0); lds_bytes: the LDS budget of the
        tile rule and the whole-mesh tests (0: device default); -1 keeps a setting"""
        self._chk(lib().scema_md_pppm_tiling(self.h, C.c_int32(mode), C.c_int32(lds_bytes)))

    def pppm_binning(self, mode: int = -1):
        """binned charge assignment: 0 off, 1 on for every eligible launch, 2 (default) by the launch policy; -1 keeps"""
        self._chk(lib().scema_md_pppm_binning(self.h, C.c_int32(mode)))

    def bonded_grouping(self, mode: int = -1):
        """stream of the bonded kernel: 0 one descriptor per term, 1 grouped (dihedrals per central bond, 1-2 / 1-3 pairs in their host term), -1 the default (grouped)"""
        self._chk(lib().scema_md_bonded_grouping(self.h, C.c_int32(mode)))

    def pppm_force_layout(self, mode: int = -1):
        """LDS layout of the staged interpolation kernel: 0 dense, 1 the stride rule of md_pppm_fstride.h, -1 the default (the rule)"""
        self._chk(lib().scema_md_pppm_force_layout(self.h, C.c_int32(mode)))

    def pppm_binned_launches(self) -> int:
        """spreading launches that took the binned kernels so far"""
        lib().scema_md_pppm_binned_launches.restype = C.c_longlong
        return int(lib().scema_md_pppm_binned_launches(self.h))

    def pppm_paths(self) -> dict:
        """what the last PPPM launch group took: spread 0 whole / 1 tiled / 2 global atomics, force 0 staged / 1 tiled / 2 unstaged,
        the largest tile counts (y, z) of either, the LDS budget in force and the mode"""
        out = (C.c_int32 * 8)()
        self._chk(lib().scema_md_pppm_paths(self.h, out))
        return dict(spread=int(out[0]), force=int(out[1]), spread_tiles=(int(out[2]), int(out[3])), force_tiles=(int(out[4]), int(out[5])),
                    lds_bytes=int(out[6]), mode=int(out[7]))

    def concurrency(self) -> dict:
        """the current issue settings: {"split": 0/1, "reax_halves": n, "reax_overlap": 0/1}"""
        out = (C.c_int32 * 3)()
        self._chk(lib().scema_md_get_concurrency(self.h, out))
        return dict(split=int(out[0]), reax_halves=int(out[1]), reax_overlap=int(out[2]))

    def reax_compute(self, matid, replica, qp=QP_NONE):
        n = self._natoms[(matid, replica)]
        f = np.zeros((n, 3)); e = np.zeros(len(REAX_PARTS)); w = np.zeros(6); q = np.zeros(n); info = np.zeros(6)
        self._chk(lib().scema_md_reax_debug_compute(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(f), _p(e), _p(w), _p(q), _p(info)))
        return dict(f=f, e=dict(zip(REAX_PARTS, e)), w=w, q=q, maxneigh_seen=int(info[0]), maxnb=int(info[1]), maxbd=int(info[2]),
                    qeq_iters=int(info[3]), image_search=int(info[4]), maxbonds_seen=int(info[5]))

    # ---- replicas under a potential on full neighbour rows: pair_style sw, tersoff, eam/alloy ----
    def _row_configure(self, symbol, matid, path, elements, energy_unit, skin):
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self._chk(getattr(lib(), symbol)(self.h, matid.encode(), path.encode(), arr, C.c_int32(len(elements)), C.c_int32(energy_unit), C.c_double(skin)))

    def _row_compute(self, symbol, matid, replica, qp, ea_key, eb_key, count_key):
        n = self.natoms(matid, replica)
        f = np.zeros((n, 3)); ea = C.c_double(0.0); eb = C.c_double(0.0); w = np.zeros(6); info = np.zeros(4)
        self._chk(getattr(lib(), symbol)(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(f), C.byref(ea), C.byref(eb), _p(w), _p(info)))
        return {"f": f, ea_key: ea.value, eb_key: eb.value, "w": w, "maxrow": int(info[0]), "rowcap": int(info[1]), "npairs": int(info[2]),
                count_key: int(info[3])}

    def sw_configure(self, matid: str, sw_path: str, elements=("Si",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style sw + pair_coeff * * <sw_path> <elements> for the replicas of one material id (lammps_scripts_sisw/in.strain.lammps);
        energy_unit 0: the file's epsilon is eV, 1: kcal/mol as written"""
        self._row_configure("scema_md_sw_configure", matid, sw_path, elements, energy_unit, skin)

    def sw_compute(self, matid, replica, qp=QP_NONE):
        return self._row_compute("scema_md_sw_debug_compute", matid, replica, qp, "e2", "e3", "ntriplets")

    def tersoff_configure(self, matid: str, path: str, elements=("Si",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style tersoff + pair_coeff * * <path> <elements> for the replicas of one material id; energy_unit 0: the file's A and B are
        eV, 1: kcal/mol as written.  Replaces a Stillinger-Weber potential of the material"""
        self._row_configure("scema_md_tersoff_configure", matid, path, elements, energy_unit, skin)

    def tersoff_compute(self, matid, replica, qp=QP_NONE):
        return self._row_compute("scema_md_tersoff_debug_compute", matid, replica, qp, "e_rep", "e_att", "nzeta")

    def tersoff_mod_configure(self, matid: str, path: str, elements=("Si",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style tersoff/mod or tersoff/mod/c (a file whose first entry has 18 numbers) + pair_coeff * * <path> <elements>; energy_unit
        as for tersoff_configure.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_tersoff_mod_configure", matid, path, elements, energy_unit, skin)

    def tersoff_mod_compute(self, matid, replica, qp=QP_NONE):
        return self._row_compute("scema_md_tersoff_mod_debug_compute", matid, replica, qp, "e_rep", "e_att", "nzeta")

    def tersoff_zbl_configure(self, matid: str, path: str, elements=("Si",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style tersoff/zbl + pair_coeff * * <path> <elements>; energy_unit 0: A, B in eV, 1: kcal/mol as written, with the Coulomb
        constant of `units real`.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_tersoff_zbl_configure", matid, path, elements, energy_unit, skin)

    def tersoff_zbl_compute(self, matid, replica, qp=QP_NONE):
        return self._row_compute("scema_md_tersoff_zbl_debug_compute", matid, replica, qp, "e_rep", "e_att", "nzeta")

    def vashishta_configure(self, matid: str, path: str, elements=("Si", "C"), energy_unit: int = 0, skin: float = -1.0):
        """pair_style vashishta + pair_coeff * * <path> <elements> for the replicas of one material id; energy_unit 0: H, D, W and B are
        eV-based with K = 14.399645 eV A, 1: kcal/mol as written with K = 332.06371.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_vashishta_configure", matid, path, elements, energy_unit, skin)

    def vashishta_compute(self, matid, replica, qp=QP_NONE):
        """npairs: ordered pairs inside rc; ntriplets: pairs (a, b) of the lists inside r0"""
        return self._row_compute("scema_md_vashishta_debug_compute", matid, replica, qp, "e2", "e3", "ntriplets")

    vashishta_debug_compute = vashishta_compute

    def eam_configure(self, matid: str, path: str, elements=("Cu",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style eam/alloy + pair_coeff * * <path> <elements> for the replicas of one material id (a DYNAMO setfl file); energy_unit 0:
        the file's F and r phi are eV, 1: kcal/mol as written.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_eam_configure", matid, path, elements, energy_unit, skin)

    def eam_compute(self, matid, replica, qp=QP_NONE):
        return self._row_compute("scema_md_eam_debug_compute", matid, replica, qp, "e_pair", "e_embed", "nabove")

    def edip_configure(self, matid: str, path: str, elements=("Si",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style edip (edip/multi) + pair_coeff * * <path> <elements> for the replicas of one material id; energy_unit 0: A and lambda
        are eV, 1: kcal/mol as written.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_edip_configure", matid, path, elements, energy_unit, skin)

    def edip_compute(self, matid, replica, qp=QP_NONE):
        """npairs: ordered pairs inside a (cutoffA); ntriplets: pairs (a, b) of the lists inside a"""
        return self._row_compute("scema_md_edip_debug_compute", matid, replica, qp, "e2", "e3", "ntriplets")

    edip_debug_compute = edip_compute

    def meam_spline_configure(self, matid: str, path: str, elements=("Ti",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style meam/spline + pair_coeff * * <path> <elements> for the replicas of one material id (either file format); energy_unit 0:
        phi and U are eV, 1: kcal/mol as written.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_meam_spline_configure", matid, path, elements, energy_unit, skin)

    def meam_spline_compute(self, matid, replica, qp=QP_NONE):
        """npairs: ordered pairs inside cutmax; ntriplets: pairs (a, b) of the lists inside f's last knot"""
        return self._row_compute("scema_md_meam_spline_debug_compute", matid, replica, qp, "e_pair", "e_embed", "ntriplets")

    meam_spline_debug_compute = meam_spline_compute

    def born_dsf_configure(self, matid: str, path: str, energy_unit: int = 0, skin: float = -1.0):
        """pair_style born/coul/dsf for the replicas of one material id: `path` is a text file with the script lines themselves (pair_style
        born/coul/dsf alpha cut_lj [cut_coul]; pair_coeff I J A rho sigma C D [cut_lj]; optionally units real|metal); energy_unit 0: A, C
        and D are eV-based with K = 14.399645 eV A, 1: kcal/mol as written with K = 332.06371.  The charges are those of the registered
        replica (ionic_system).  Replaces whatever potential the material held"""
        self._chk(lib().scema_md_born_dsf_configure(self.h, matid.encode(), path.encode(), C.c_int32(energy_unit), C.c_double(skin)))

    def born_dsf_compute(self, matid, replica, qp=QP_NONE):
        """e_coul holds the self term; npairs: ordered pairs inside cutmax; ncoul: ordered pairs inside cut_coul"""
        return self._row_compute("scema_md_born_dsf_debug_compute", matid, replica, qp, "e_born", "e_coul", "ncoul")

    born_dsf_debug_compute = born_dsf_compute

    def born_long_configure(self, matid: str, path: str, energy_unit: int = 0, skin: float = -1.0):
        """pair_style born/coul/long or buck/coul/long with an Ewald sum for the replicas of one material id: `path` is a text file with the
        script lines themselves (pair_style born/coul/long cut_lj [cut_coul] with pair_coeff I J A rho sigma C D [cut_lj], or buck/coul/long
        with pair_coeff I J A rho C [cut_lj]; kspace_style ewald|pppm accuracy; optionally units real|metal); energy_unit as for
        born_dsf_configure.  The charges are those of the registered replica (ionic_system).  Replaces whatever potential the material held"""
        self._chk(lib().scema_md_born_long_configure(self.h, matid.encode(), path.encode(), C.c_int32(energy_unit), C.c_double(skin)))

    def born_long_compute(self, matid, replica, qp=QP_NONE):
        """e_coul: real space, reciprocal space, self and background; npairs: ordered pairs inside cutmax; ncoul: ordered pairs inside
        cut_coul; nk: k-vectors of the half space; g_ewald of the evaluation"""
        n = self.natoms(matid, replica)
        f = np.zeros((n, 3)); ea = C.c_double(0.0); eb = C.c_double(0.0); w = np.zeros(6); info = np.zeros(6)
        self._chk(lib().scema_md_born_long_debug_compute(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(f), C.byref(ea), C.byref(eb), _p(w),
                                                         _p(info)))
        return {"f": f, "e_born": ea.value, "e_coul": eb.value, "w": w, "maxrow": int(info[0]), "rowcap": int(info[1]), "npairs": int(info[2]),
                "ncoul": int(info[3]), "nk": int(info[4]), "g_ewald": float(info[5])}

    born_long_debug_compute = born_long_compute

    def born_long_kspace(self, matid: str, mode: int = 0):
        """the reciprocal solver of a Born/long material's replicas: 0 by the script and the Ewald limits (the Ewald sum where its k list
        fits; beyond it a `pppm` script runs on the mesh and an `ewald` script is refused), 1 the PPPM mesh for every replica, 2 the Ewald
        sum always.  On the mesh born_long_compute reports nk 0 and the adjusted g_ewald"""
        self._chk(lib().scema_md_born_long_kspace(self.h, matid.encode(), C.c_int32(mode)))

    def born_long_mesh_configure(self, matid: str, path: str, energy_unit: int = 0, skin: float = -1.0):
        """born_long_configure, then the mesh solver for every replica of the material (born_long_kspace mode 1)"""
        self.born_long_configure(matid, path, energy_unit, skin)
        self.born_long_kspace(matid, 1)

    def born_long_last_mesh(self):
        """the mesh (nx, ny, nz) of the last born_long_compute, zeros if it ran the Ewald sum"""
        grid = np.zeros(3, np.int32)
        self._chk(lib().scema_md_born_long_last_mesh(self.h, _p(grid)))
        return tuple(int(v) for v in grid)

    def eam_coul_configure(self, matid: str, path: str, energy_unit: int = 0, skin: float = -1.0):
        """pair_style hybrid/overlay coul/long <cut_coul> eam/alloy for the replicas of one material id: `path` is a text file with the
        script lines themselves (that pair_style line, pair_coeff * * coul/long, pair_coeff * * eam/alloy <file> <El> ..., kspace_style
        ewald|pppm accuracy; optionally units real|metal); <file> is taken relative to the script's folder unless absolute; energy_unit 0:
        the setfl tables are eV, K = 14.399645 eV A, 1: kcal/mol as written, K = 332.06371.  The charges are those of the registered
        replica (ionic_system).  Replaces whatever potential the material held"""
        self._chk(lib().scema_md_eam_coul_configure(self.h, matid.encode(), path.encode(), C.c_int32(energy_unit), C.c_double(skin)))

    def eam_coul_compute(self, matid, replica, qp=QP_NONE):
        """e_eam: embedding and pair energy; e_coul: real space, reciprocal space, self and background; npairs: ordered pairs inside the
        setfl cutoff; ncoul: ordered pairs inside cut_coul; nk: k-vectors of the half space; g_ewald of the evaluation"""
        n = self.natoms(matid, replica)
        f = np.zeros((n, 3)); ea = C.c_double(0.0); eb = C.c_double(0.0); w = np.zeros(6); info = np.zeros(6)
        self._chk(lib().scema_md_eam_coul_debug_compute(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), _p(f), C.byref(ea), C.byref(eb), _p(w),
                                                        _p(info)))
        return {"f": f, "e_eam": ea.value, "e_coul": eb.value, "w": w, "maxrow": int(info[0]), "rowcap": int(info[1]), "npairs": int(info[2]),
                "ncoul": int(info[3]), "nk": int(info[4]), "g_ewald": float(info[5])}

    eam_coul_debug_compute = eam_coul_compute

    def eam_coul_kspace(self, matid: str, mode: int = 0):
        """the reciprocal solver of an EAM/coul material's replicas: the three modes of born_long_kspace"""
        self._chk(lib().scema_md_eam_coul_kspace(self.h, matid.encode(), C.c_int32(mode)))

    def eam_coul_last_mesh(self):
        """the mesh (nx, ny, nz) of the last eam_coul_compute, zeros if it ran the Ewald sum"""
        grid = np.zeros(3, np.int32)
        self._chk(lib().scema_md_eam_coul_last_mesh(self.h, _p(grid)))
        return tuple(int(v) for v in grid)

    def adp_configure(self, matid: str, path: str, elements=("Cu",), energy_unit: int = 0, skin: float = -1.0):
        """pair_style adp + pair_coeff * * <path> <elements> for the replicas of one material id (an extended setfl file); energy_unit 0: F
        and r phi are eV, u and w the square root of eV per A and per A^2; 1: kcal/mol as written.  Replaces whatever potential the material held"""
        self._row_configure("scema_md_adp_configure", matid, path, elements, energy_unit, skin)

    def adp_compute(self, matid, replica, qp=QP_NONE):
        """e_pair: 1/2 sum phi; e_manybody: the embedding energy plus the angular terms; nabove: atoms above rhomax"""
        return self._row_compute("scema_md_adp_debug_compute", matid, replica, qp, "e_pair", "e_manybody", "nabove")

    # ---- init_material's equilibration schedule (in.init.lammps; md_equil.hip) ----
    def minimize(self, matid, replica, qp, etol=1e-7, ftol=1e-11, maxiter=1000, maxeval=50000) -> dict:
        info = np.zeros(5)
        self._chk(lib().scema_md_debug_minimize(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), C.c_double(etol), C.c_double(ftol),
                                                C.c_int32(maxiter), C.c_int32(maxeval), _p(info)))
        return dict(stop=int(info[0]), iterations=int(info[1]), evaluations=int(info[2]), e_initial=info[3], e_final=info[4])

    def run_nh(self, matid, replica, qp, nsteps, dt, t_start, t_stop=None, npt=False, p_target=1.0, p_period=1000.0, average_lengths=False):
        lav = np.zeros(3) if average_lengths else None
        self._chk(lib().scema_md_debug_run_nh(self.h, C.c_int32(qp), matid.encode(), C.c_int32(replica), C.c_int32(nsteps), C.c_double(dt),
                                              C.c_double(t_start), C.c_double(t_start if t_stop is None else t_stop), C.c_int32(1 if npt else 0),
                                              C.c_double(p_target), C.c_double(p_period), _p(lav) if average_lengths else None))
        return lav

    def equilibrate(self, matid, replica, nsteps_equil, dt, temperature, seed=1234):
        p = EquilParams(nsteps_equil, dt, temperature, seed)
        length, info = np.zeros(3), np.zeros(5)
        self._chk(lib().scema_md_equilibrate(self.h, matid.encode(), C.c_int32(replica), C.byref(p), _p(length), _p(info)))
        return length, dict(stop=int(info[0]), iterations=int(info[1]), evaluations=int(info[2]), e_initial=info[3], e_final=info[4])

    def reax_stats(self) -> dict:
        out = np.zeros(7)
        self._chk(lib().scema_md_reax_stats(self.h, _p(out)))
        return dict(qeq_iters=int(out[0]), qeq_solves=int(out[1]), skin=out[2], qeq_tol=out[3], qeq_slow_solves=int(out[4]),
                    qeq_launched_iters=int(out[5]), precond_fallbacks=int(out[6]))

    def profile(self, reset=False) -> dict:
        p = Profile()
        self._chk(lib().scema_md_get_profile(self.h, C.byref(p), C.c_int32(1 if reset else 0)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}


def env_overrides() -> list:
    """the library's declared environment switches that are set in this process ("NAME=value"); empty in a clean run"""
    buf = C.create_string_buffer(4096)
    lib().scema_md_env_overrides.restype = C.c_int
    n = lib().scema_md_env_overrides(buf, C.c_int(len(buf)))
    return [l for l in buf.value.decode().split("\n") if l] if n else []


def box_fp64_tflops(device: int = 0) -> float:
    """FP64 FMA ceiling of the device as measured now (scema_md_box_fma_tflops): the calibration bench.py prints beside its rates"""
    out = C.c_double(0.0)
    lib().scema_md_box_fma_tflops.restype = C.c_int
    rc = lib().scema_md_box_fma_tflops(C.c_int32(device), C.byref(out))
    if rc:
        raise EngineError(f"scema_md_box_fma_tflops failed with code {rc} (no HIP device?)")
    return float(out.value)


def sw_system(types, x, box, v=None, masses=(28.0855,)) -> dict:
    """System dict of a Stillinger-Weber replica (atom_style atomic): LAMMPS types (0-based here) and masses only -- no charges, no
    topology, zero Lennard-Jones coefficients"""
    n = len(types)
    nt = len(masses)
    z2 = np.zeros((0, 2))
    return dict(natoms=n, ntypes=nt, type=np.asarray(types, np.int32), charge=np.zeros(n), mass=np.array(masses, float),
                eps=np.zeros((nt, nt)), sigma=np.ones((nt, nt)), bonds=np.zeros((0, 2), np.int32), bond_type=np.zeros(0, np.int32), bond_coeff=z2,
                angles=np.zeros((0, 3), np.int32), angle_type=np.zeros(0, np.int32), angle_coeff=z2, dihedrals=np.zeros((0, 4), np.int32),
                dihedral_type=np.zeros(0, np.int32), dihedral_coeff=np.zeros((0, 4)), impropers=np.zeros((0, 4), np.int32),
                improper_type=np.zeros(0, np.int32), improper_coeff=z2, special_lj=np.zeros(3), special_coul=np.zeros(3),
                box=np.asarray(box, float), x=np.asarray(x, float), v=np.zeros((n, 3)) if v is None else np.asarray(v, float))


bare_system = sw_system   # (the same bare replica under a neutral name: what a Tersoff or an embedded-atom material registers too)


def ionic_system(types, charges, x, box, masses, v=None) -> dict:
    """System dict of an ionic replica (atom_style charge): LAMMPS types (0-based here), a charge per atom and masses -- no topology, zero
    Lennard-Jones coefficients: what a born/coul/dsf material registers"""
    s = sw_system(types, x, box, v=v, masses=tuple(masses))
    q = np.asarray(charges, float)
    if q.shape != (len(types),):
        raise ValueError("ionic_system: one charge per atom")
    s["charge"] = q.copy()
    return s


BORN_DSF_FIELDS = ["A", "rho", "sigma", "C", "D", "cut_lj"]
BD_MAXEL = 4


def born_dsf_read_params(path: str, energy_unit: int = 0):
    """dict of the born/coul/dsf lines of a text file (scema_md_born_dsf_read_params, a pure host function, no GPU): n (the fragment's
    types), alpha, cut_coul, e_s, f_s, K (kcal A/mol), cutmax, and values[n][n][6] in the order of BORN_DSF_FIELDS, A, C and D in kcal/mol;
    raises IOError with the reader's message, which names the line"""
    read = lib().scema_md_born_dsf_read_params
    read.restype = C.c_int
    nt = C.c_int32(0)
    head, vals = np.zeros(6), np.zeros(BD_MAXEL * BD_MAXEL * len(BORN_DSF_FIELDS))
    err = C.create_string_buffer(512)
    rc = read(path.encode(), C.c_int32(energy_unit), C.byref(nt), _p(head), _p(vals), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    n = nt.value
    return dict(n=n, alpha=head[0], cut_coul=head[1], e_s=head[2], f_s=head[3], K=head[4], cutmax=head[5],
                values=vals[:n * n * len(BORN_DSF_FIELDS)].reshape(n, n, len(BORN_DSF_FIELDS)).copy())


def born_dsf_eval(path: str, ti: int, tj: int, qi: float, qj: float, r, energy_unit: int = 0):
    """(e_born, e_coul, fb, fc) at the distances r and the two self energies, by the code the kernel runs (scema_md_born_dsf_eval, a pure
    host function): the force on i is -(fb + fc) (x_j - x_i)"""
    ev = lib().scema_md_born_dsf_eval
    ev.restype = C.c_int
    r = np.ascontiguousarray(r, float).ravel()
    out, eself = np.zeros((len(r), 4)), np.zeros(2)
    err = C.create_string_buffer(512)
    rc = ev(path.encode(), C.c_int32(energy_unit), C.c_int32(ti), C.c_int32(tj), C.c_double(qi), C.c_double(qj), _p(r), C.c_int32(len(r)), _p(out),
            _p(eself), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3], eself


def born_long_read_params(path: str, energy_unit: int = 0):
    """dict of the born/coul/long or buck/coul/long lines of a text file (scema_md_born_long_read_params, a pure host function, no GPU): n,
    cut_coul, accuracy, solver ("ewald" or "pppm"), K (kcal A/mol), cutmax, style ("born" or "buck") and values[n][n][6] in the order of
    BORN_DSF_FIELDS, A, C and D in kcal/mol; raises IOError with the reader's message, which names the line"""
    read = lib().scema_md_born_long_read_params
    read.restype = C.c_int
    nt = C.c_int32(0)
    head, vals = np.zeros(6), np.zeros(BD_MAXEL * BD_MAXEL * len(BORN_DSF_FIELDS))
    err = C.create_string_buffer(512)
    rc = read(path.encode(), C.c_int32(energy_unit), C.byref(nt), _p(head), _p(vals), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    n = nt.value
    return dict(n=n, cut_coul=head[0], accuracy=head[1], solver="pppm" if head[2] else "ewald", K=head[3], cutmax=head[4],
                style="buck" if head[5] else "born", values=vals[:n * n * len(BORN_DSF_FIELDS)].reshape(n, n, len(BORN_DSF_FIELDS)).copy())


def born_long_eval(path: str, g_ewald: float, ti: int, tj: int, qi: float, qj: float, r, energy_unit: int = 0):
    """(e_born, e_real, fb, fc) at the distances r for that g_ewald, by the code the kernel runs (scema_md_born_long_eval, a pure host
    function): the force on i is -(fb + fc) (x_j - x_i)"""
    ev = lib().scema_md_born_long_eval
    ev.restype = C.c_int
    r = np.ascontiguousarray(r, float).ravel()
    out = np.zeros((len(r), 4))
    err = C.create_string_buffer(512)
    rc = ev(path.encode(), C.c_int32(energy_unit), C.c_double(g_ewald), C.c_int32(ti), C.c_int32(tj), C.c_double(qi), C.c_double(qj), _p(r),
            C.c_int32(len(r)), _p(out), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def born_long_kvectors(path: str, box, natoms: int, qsqsum: float, energy_unit: int = 0):
    """the k-space set-up a run would use for that box (scema_md_born_long_kvectors, a pure host function): dict g_ewald, kmax (3), nk,
    triples [nk][3]"""
    kv = lib().scema_md_born_long_kvectors
    kv.restype = C.c_int
    box = np.ascontiguousarray(box, float)
    g, kmax, nk = C.c_double(0.0), np.zeros(3, np.int32), C.c_int32(0)
    err = C.create_string_buffer(512)
    args = (path.encode(), C.c_int32(energy_unit), _p(box), C.c_int32(natoms), C.c_double(qsqsum), C.byref(g), _p(kmax), C.byref(nk))
    rc = kv(*args, None, C.c_int32(0), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    tr = np.zeros((max(nk.value, 1), 3), np.int32)
    rc = kv(*args, _p(tr), C.c_int32(len(tr)), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return dict(g_ewald=g.value, kmax=kmax.copy(), nk=nk.value, triples=tr[:nk.value].copy())


def born_long_mesh(path: str, box, natoms: int, qsqsum: float, energy_unit: int = 0):
    """the mesh set-up a run on the mesh solver would use for that box (scema_md_born_long_mesh, a pure host function): dict g_ewald,
    grid (3); a mesh the solver refuses raises IOError with the refusal"""
    fn = lib().scema_md_born_long_mesh
    fn.restype = C.c_int
    box = np.ascontiguousarray(box, float)
    g, grid = C.c_double(0.0), np.zeros(3, np.int32)
    err = C.create_string_buffer(512)
    rc = fn(path.encode(), C.c_int32(energy_unit), _p(box), C.c_int32(natoms), C.c_double(qsqsum), C.byref(g), _p(grid), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return dict(g_ewald=g.value, grid=tuple(int(v) for v in grid))


def eam_coul_read_params(path: str, energy_unit: int = 0):
    """dict of the hybrid/overlay coul/long eam/alloy lines of a text file and the setfl file it names (scema_md_eam_coul_read_params, a
    pure host function, no GPU): cut_coul, accuracy, solver ("ewald" or "pppm"), K (kcal A/mol), cutmax, cutoff (of the setfl file),
    type_map (element of the tables per atom type) and setfl (the resolved path); raises IOError with the reader's message"""
    read = lib().scema_md_eam_coul_read_params
    read.restype = C.c_int
    head, nt, tmap = np.zeros(6), C.c_int32(0), np.zeros(64, np.int32)
    setfl, err = C.create_string_buffer(4096), C.create_string_buffer(512)
    rc = read(path.encode(), C.c_int32(energy_unit), _p(head), C.byref(nt), _p(tmap), C.c_int32(len(tmap)), setfl, C.c_int32(len(setfl)), err,
              C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return dict(cut_coul=head[0], accuracy=head[1], solver="pppm" if head[2] else "ewald", K=head[3], cutmax=head[4], cutoff=head[5],
                type_map=[int(v) for v in tmap[:min(nt.value, len(tmap))]], setfl=setfl.value.decode())


SW_FIELDS = ["epsilon", "sigma", "a", "lambda", "gamma", "costheta0", "A", "B", "p", "q", "tol"]
TERSOFF_FIELDS = ["m", "gamma", "lambda3", "c", "d", "costheta0", "n", "beta", "lambda2", "B", "R", "D", "lambda1", "A"]
TERSOFF_MOD_FIELDS = ["beta", "alpha", "h", "eta", "beta_ters", "lambda2", "B", "R", "D", "lambda1", "A", "n", "c1", "c2", "c3", "c4", "c5", "c0"]
TERSOFF_ZBL_FIELDS = TERSOFF_FIELDS + ["Z_i", "Z_j", "ZBLcut", "ZBLexpscale"]
EDIP_FIELDS = ["A", "B", "cutoffA", "cutoffC", "alpha", "beta", "eta", "gamma", "lambda", "mu", "rho", "sigma", "Q0", "u1", "u2", "u3", "u4"]
VASHISHTA_FIELDS = ["H", "eta", "Zi", "Zj", "lambda1", "D", "lambda4", "W", "rc", "B", "gamma", "r0", "C", "costheta0"]


def _read_triplet_params(symbol: str, nfields: int, path: str, elements, energy_unit: int):
    fn = getattr(lib(), symbol)
    fn.restype = C.c_int
    arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
    nk = C.c_int32(0)
    tmap = np.zeros(len(elements), np.int32)
    vals = np.zeros(4 * 4 * 4 * nfields)
    err = C.create_string_buffer(512)
    rc = fn(path.encode(), arr, C.c_int32(len(elements)), C.c_int32(energy_unit), C.byref(nk), _p(tmap), _p(vals), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    n = nk.value
    return n, tmap, vals[:n * n * n * nfields].reshape(n, n, n, nfields).copy()


def sw_read_params(sw_path: str, elements, energy_unit: int = 0):
    """(distinct elements kept, type_map, values[n][n][n][11] in the order of SW_FIELDS, epsilon in kcal/mol) of a LAMMPS *.sw file:
    scema_md_sw_read_params, a pure host function (no GPU); raises IOError with the reader's message"""
    return _read_triplet_params("scema_md_sw_read_params", len(SW_FIELDS), sw_path, elements, energy_unit)


def tersoff_read_params(path: str, elements, energy_unit: int = 0):
    """(distinct elements kept, type_map, values[n][n][n][14] in the order of TERSOFF_FIELDS, A and B in kcal/mol) of a LAMMPS *.tersoff
    file: scema_md_tersoff_read_params, a pure host function (no GPU); raises IOError with the reader's message"""
    return _read_triplet_params("scema_md_tersoff_read_params", len(TERSOFF_FIELDS), path, elements, energy_unit)


def tersoff_mod_read_params(path: str, elements, energy_unit: int = 0):
    """as tersoff_read_params for a *.tersoff.mod or *.tersoff.modc file: values[n][n][n][18] in the order of TERSOFF_MOD_FIELDS (c0 = 0
    for a 17-column file), A, B and c0 in kcal/mol: scema_md_tersoff_mod_read_params"""
    return _read_triplet_params("scema_md_tersoff_mod_read_params", len(TERSOFF_MOD_FIELDS), path, elements, energy_unit)


def tersoff_zbl_read_params(path: str, elements, energy_unit: int = 0):
    """as tersoff_read_params for a *.tersoff.zbl file: values[n][n][n][18] in the order of TERSOFF_ZBL_FIELDS: scema_md_tersoff_zbl_read_params"""
    return _read_triplet_params("scema_md_tersoff_zbl_read_params", len(TERSOFF_ZBL_FIELDS), path, elements, energy_unit)


def edip_read_params(path: str, elements, energy_unit: int = 0):
    """(distinct elements kept, type_map, values[n][n][n][17] in the order of EDIP_FIELDS, A and lambda in kcal/mol) of a LAMMPS *.edip
    file: scema_md_edip_read_params, a pure host function (no GPU); raises IOError with the reader's message"""
    return _read_triplet_params("scema_md_edip_read_params", len(EDIP_FIELDS), path, elements, energy_unit)


MS_MAXEL, MS_MAXKNOT = 2, 32
MS_NFN = MS_MAXEL * (MS_MAXEL + 1) + 3 * MS_MAXEL


def _ms_elements(elements):
    return (C.c_char_p * len(elements))(*[None if e is None else e.encode() for e in elements])


def meam_spline_read_params(path: str, elements, energy_unit: int = 0):
    """dict of a LAMMPS meam/spline file of either format (scema_md_meam_spline_read_params, a pure host function, no GPU): n (distinct
    elements kept), type_map, cutmax, u0[n], cut_f[n][n], and fn: the splines of the elements kept in the file's order (phi as the upper
    triangle, rho, U, f, g as the upper triangle), each a dict n, d0, dn, uniform, ih, x, y, y2 with phi and U in kcal/mol; raises IOError
    with the reader's message"""
    read = lib().scema_md_meam_spline_read_params
    read.restype = C.c_int
    nk = C.c_int32(0)
    tmap = np.zeros(len(elements), np.int32)
    knots = np.zeros(MS_NFN, np.int32)
    head = np.zeros(2 + MS_MAXEL + MS_MAXEL * MS_MAXEL)
    stride = 4 + 3 * MS_MAXKNOT
    vals = np.zeros(MS_NFN * stride)
    err = C.create_string_buffer(512)
    rc = read(path.encode(), _ms_elements(elements), C.c_int32(len(elements)), C.c_int32(energy_unit), C.byref(nk), _p(tmap), _p(knots), _p(head), _p(vals),
              err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    n = nk.value
    fn = []
    for k in range(int(head[1])):
        v, m = vals[k * stride:(k + 1) * stride], int(knots[k])
        fn.append(dict(n=m, d0=v[0], dn=v[1], uniform=int(v[2]), ih=v[3], x=v[4:4 + m].copy(), y=v[4 + MS_MAXKNOT:4 + MS_MAXKNOT + m].copy(),
                       y2=v[4 + 2 * MS_MAXKNOT:4 + 2 * MS_MAXKNOT + m].copy()))
    return dict(n=n, type_map=tmap, cutmax=head[0], u0=head[2:2 + n].copy(),
                cut_f=head[2 + MS_MAXEL:].reshape(MS_MAXEL, MS_MAXEL)[:n, :n].copy(), fn=fn)


def meam_spline_eval(path: str, elements, fn: int, x, energy_unit: int = 0, search: bool = False):
    """(y, dy) of spline `fn` (the order of meam_spline_read_params) of the file at the points x, evaluated by the code the kernels run
    (scema_md_meam_spline_eval, a pure host function); search: by bisection even where the knots are equidistant"""
    ev = lib().scema_md_meam_spline_eval
    ev.restype = C.c_int
    x = np.ascontiguousarray(x, float).ravel()
    y, dy = np.zeros(len(x)), np.zeros(len(x))
    err = C.create_string_buffer(512)
    rc = ev(path.encode(), _ms_elements(elements), C.c_int32(len(elements)), C.c_int32(energy_unit), C.c_int32(fn), C.c_int32(1 if search else 0), _p(x),
            C.c_int32(len(x)), _p(y), _p(dy), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    return y, dy


def vashishta_read_params(path: str, elements, energy_unit: int = 0):
    """(distinct elements kept, type_map, values[n][n][n][14] in the order of VASHISHTA_FIELDS, H, D, W and B in kcal/mol) of a LAMMPS
    *.vashishta file: scema_md_vashishta_read_params, a pure host function (no GPU); raises IOError with the reader's message"""
    return _read_triplet_params("scema_md_vashishta_read_params", len(VASHISHTA_FIELDS), path, elements, energy_unit)


def eam_read_setfl(path: str, elements, energy_unit: int = 0):
    """dict of a DYNAMO setfl file (scema_md_eam_read_setfl, a pure host function, no GPU): n (distinct elements kept), type_map, nrho,
    drho, nr, dr, cutoff, rhomax, masses[n], and the spline records F[i] (value [nrho][4] {s3 s4 s5 s6}, derivative [nrho][4] {s0 s1 s2
    0}), rho[i], z[(i, j)] (r phi, i >= j) as pairs of arrays, F and r phi in kcal/mol; raises IOError with the reader's message"""
    return _read_setfl("scema_md_eam_read_setfl", False, path, elements, energy_unit)


def adp_read_setfl(path: str, elements, energy_unit: int = 0):
    """the dict of eam_read_setfl for an extended setfl file of pair_style adp (scema_md_adp_read_setfl), with u[(i, j)] and w[(i, j)],
    i >= j, besides: the records of the dipole and quadrupole functions, in the square root of kcal/mol per A and per A^2"""
    return _read_setfl("scema_md_adp_read_setfl", True, path, elements, energy_unit)


def _read_setfl(symbol: str, adp: bool, path: str, elements, energy_unit: int):
    L = lib()
    read = getattr(L, symbol)
    read.restype = C.c_int
    arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
    nk = C.c_int32(0)
    tmap = np.zeros(len(elements), np.int32)
    head, masses = np.zeros(8), np.zeros(4)
    err = C.create_string_buffer(512)
    args = (path.encode(), arr, C.c_int32(len(elements)), C.c_int32(energy_unit), C.byref(nk), _p(tmap), _p(head), _p(masses))
    rc = read(*args, None, C.c_int64(0), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    tab = np.zeros(int(head[6]))
    rc = read(*args, _p(tab), C.c_int64(len(tab)), err, C.c_int32(len(err)))
    if rc != 0:
        raise IOError(f"rc={rc}: {err.value.decode(errors='replace')}")
    n, nrho, nr = nk.value, int(head[0]), int(head[2])
    pos = 0

    def take(m):
        nonlocal pos
        val, der = tab[pos:pos + 4 * m].reshape(m, 4).copy(), tab[pos + 4 * m:pos + 8 * m].reshape(m, 4).copy()
        pos += 8 * m
        return val, der
    F, rho, z = [], [], {}
    for _ in range(n):
        F.append(take(nrho))
        rho.append(take(nr))
    for i in range(n):
        for j in range(i + 1):
            z[(i, j)] = take(nr)
    out = dict(n=n, type_map=tmap, nrho=nrho, drho=head[1], nr=nr, dr=head[3], cutoff=head[4], rhomax=head[5], masses=masses[:n].copy(), F=F, rho=rho, z=z)
    if adp:
        for key in ("u", "w"):
            out[key] = {(i, j): take(nr) for i in range(n) for j in range(i + 1)}
    assert pos == len(tab)
    return out


def kspace_setup(params, box, qsqsum: float, natoms: int):
    """(g_initial, g_ewald, grid) a run would use for this box: scema_md_kspace_setup, a pure host function (no GPU)"""
    L = lib()
    L.scema_md_kspace_setup.restype = C.c_int
    b = np.ascontiguousarray(box, np.float64)
    g0, g1 = C.c_double(0.0), C.c_double(0.0)
    grid = (C.c_int32 * 3)()
    rc = L.scema_md_kspace_setup(C.byref(params), _p(b), C.c_double(qsqsum), C.c_int32(natoms), C.byref(g0), C.byref(g1), grid)
    if rc != 0:
        raise EngineError(f"scema_md_kspace_setup rc={rc}")
    return g0.value, g1.value, tuple(grid)


def pppm_tile_shape(grid, lds_bytes: int = 0, which: int = 0):
    """(by, bz, tiles_y, tiles_z) of the tiled PPPM kernels for this mesh and LDS budget (0: device default), which = 0 charge assignment,
    1 interpolation; zeros: the smallest brick does not fit.  scema_md_pppm_tile_shape, a pure host function (no GPU)"""
    L = lib()
    L.scema_md_pppm_tile_shape.restype = C.c_int
    g = (C.c_int32 * 3)(*[int(n) for n in grid])
    out = (C.c_int32 * 4)()
    rc = L.scema_md_pppm_tile_shape(g, C.c_int32(lds_bytes), C.c_int32(which), out)
    if rc != 0:
        raise EngineError(f"scema_md_pppm_tile_shape rc={rc}")
    return tuple(int(v) for v in out)


def pppm_force_strides(grid, lds_bytes: int = 0):
    """(row stride, plane stride, LDS bytes) of the staged interpolation kernel's field copy for this mesh and LDS budget (0: device
    default) by the rule of md_pppm_fstride.h.  scema_md_pppm_force_strides, a pure host function (no GPU)"""
    L = lib()
    L.scema_md_pppm_force_strides.restype = C.c_int
    g = (C.c_int32 * 3)(*[int(n) for n in grid])
    out = (C.c_int32 * 3)()
    rc = L.scema_md_pppm_force_strides(g, C.c_int32(lds_bytes), out)
    if rc != 0:
        raise EngineError(f"scema_md_pppm_force_strides rc={rc}")
    return tuple(int(v) for v in out)


def make_sim(qp_id: int, matid: str, replica: int, strain_len, *, most_recent: int | None = None, material: int = 0,
             dt=2.0, temperature=300.0, strain_rate=1e-4, nss=100, force_field="opls", stiffness=None,
             time_id="0-0", output_folder="", restart_folder="", scripts_folder="", log_file="none",
             checkpoint=False) -> MDSim:
    m = MDSim()
    m.qp_id = qp_id
    m.most_recent_qp_id = qp_id if most_recent is None else most_recent
    m.replica = replica
    m.material = material
    m.matid = matid.encode(); m.time_id = time_id.encode(); m.output_folder = output_folder.encode()
    m.restart_folder = restart_folder.encode(); m.scripts_folder = scripts_folder.encode()
    m.log_file = log_file.encode(); m.force_field = force_field.encode()
    m.strain[:] = list(np.asarray(strain_len, float))
    if stiffness is not None:
        m.stiffness[:] = list(np.asarray(stiffness, float).ravel())
    m.timestep_length = dt; m.temperature = temperature; m.strain_rate = strain_rate
    m.nsteps_sample = nss
    m.output_homog = 0
    m.checkpoint = 1 if checkpoint else 0
    return m


class PlanDir:
    """The planner alone (scema_plan_* of include/scema_md.h; pure host arithmetic, runs without a GPU)."""

    def __init__(self):
        self.h = C.c_void_p(lib().scema_plan_dir_create())

    def __del__(self):
        try:
            if self.h:
                lib().scema_plan_dir_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def update(self, sims, world: int, cost=None, commit: bool = True):
        arr = (MDSim * len(sims))(*sims) if not isinstance(sims, C.Array) else sims
        n = len(arr)
        owner = np.zeros(n, np.int32); pos = np.zeros(n, np.int32); cap = C.c_int32(0)
        moves = np.zeros((max(n, 1), 3), np.int32); nm = C.c_int32(0)
        c = None if cost is None else np.ascontiguousarray(cost, np.float64)
        rc = lib().scema_plan_update(self.h, arr, C.c_int32(n), _p(c), C.c_int32(world), _p(owner), _p(pos), C.byref(cap), _p(moves),
                                     C.byref(nm), C.c_int32(1 if commit else 0))
        if rc != 0:
            raise EngineError(f"scema_plan_update rc={rc}")
        return owner, pos, cap.value, moves[:nm.value].copy()
