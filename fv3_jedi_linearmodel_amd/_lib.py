"""ctypes binding of the C-ABI in include/fv3lm.h.

`load_hip_library()` loads the product library libfv3lm_hip.so and raises if it is missing — the
package has no CPU path.  `Fv3LmLibrary(path)` is the thin object wrapper the tests also use to
drive the test-only host-emulation build of the same sources.
"""
import ctypes as C
import os
import numpy as np
from .config import Options, Dims

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfv3lm_hip.so")
_dp = C.POINTER(C.c_double)


class Fv3LmError(RuntimeError):
    pass


class BlParams(C.Structure):
    """fv3lm_bl_params: TURBPARAMS(22), TURBPARAMSI(4) of BL_DRIVER in the reference's order"""
    _fields_ = [("r", C.c_double * 22), ("i", C.c_int * 4)]


class RasParams(C.Structure):
    """fv3lm_ras_params: RASPARAMS(1:25) of the moist physics in the reference's order"""
    _fields_ = [("r", C.c_double * 25)]


class CloudParams(C.Structure):
    """fv3lm_cloud_params: CLOUDPARAMS(1:57) of the moist physics in the reference's order"""
    _fields_ = [("r", C.c_double * 57)]


class Fv3LmLibrary:
    def __init__(self, path):
        if not os.path.exists(path):
            raise Fv3LmError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        self.path = path
        L = self.L = C.CDLL(path)
        L.fv3lm_last_error.restype = C.c_char_p
        L.fv3lm_metric_names.restype = C.c_char_p
        L.fv3lm_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Dims), C.POINTER(Options), C.POINTER(_dp),
                                   C.c_double, C.c_double, _dp, _dp, _dp]
        L.fv3lm_destroy.argtypes = [C.c_void_p]
        L.fv3lm_field_put.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _dp]
        L.fv3lm_field_get.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _dp]
        L.fv3lm_field_levels.argtypes = [C.c_void_p, C.c_char_p]
        L.fv3lm_run_group.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.fv3lm_dyn_core.argtypes = [C.c_void_p, C.c_int]
        L.fv3lm_zero_work_adjoint.argtypes = [C.c_void_p]
        L.fv3lm_sync.argtypes = [C.c_void_p]
        L.fv3lm_launch_count.argtypes = [C.c_void_p]
        L.fv3lm_launch_count.restype = C.c_long
        L.fv3lm_tp2_launch_count.argtypes = [C.c_void_p]
        L.fv3lm_tp2_launch_count.restype = C.c_long
        L.fv3lm_level_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]
        for fn in ("fv3lm_pressures", "fv3lm_tracer_2d", "fv3lm_fv_dynamics"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_int]
        L.fv3lm_remap.argtypes = [C.c_void_p, C.c_int, C.c_int]
        for fn in ("fv3lm_step_tl", "fv3lm_step_nl", "fv3lm_step_ad"):
            getattr(L, fn).argtypes = [C.c_void_p]

    def err(self):
        return self.L.fv3lm_last_error().decode()

    def metric_names(self):
        return self.L.fv3lm_metric_names().decode().split(",")


def load_hip_library():
    """The product library.  FV3LM_LIB names another build of the same HIP sources (kernel-tuning variants, tools/mkvariant.sh); a
    host-emulation build (tests/_emul, it exports fv3lm_emul_check_boxes) is refused: the package has no CPU path."""
    lib = Fv3LmLibrary(os.environ.get("FV3LM_LIB", LIB_PATH))
    if hasattr(lib.L, "fv3lm_emul_check_boxes"):
        raise Fv3LmError("%s is a host-emulation build (tests only); the package runs the HIP library alone" % lib.path)
    return lib


TRANSPORT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_dp), C.POINTER(C.c_long), C.POINTER(_dp), C.POINTER(C.c_long))


def rccl_library_path():
    """The RCCL this process already uses: torch's bundled copy if torch is imported, else the ROCm one."""
    import sys
    if "torch" in sys.modules:
        p = os.path.join(os.path.dirname(sys.modules["torch"].__file__), "lib", "librccl.so")
        if os.path.exists(p):
            return p
    return "/opt/rocm/lib/librccl.so"


def comm_init_rccl(lib, rank, world, broadcast_bytes):
    """One RCCL communicator over all ranks for the face exchange.  broadcast_bytes(buf: bytearray|None) -> bytes must hand
    rank 0's 128-byte unique id to every rank (e.g. through torch.distributed)."""
    path = rccl_library_path().encode()
    uid = C.create_string_buffer(128)
    if rank == 0:
        lib.L.fv3lm_comm_unique_id.argtypes = [C.c_char_p, C.c_void_p]
        if lib.L.fv3lm_comm_unique_id(path, uid) != 0:
            raise Fv3LmError(lib.err())
    data = broadcast_bytes(bytes(uid.raw) if rank == 0 else None)
    lib.L.fv3lm_comm_init.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    if lib.L.fv3lm_comm_init(path, data, world, rank) != 0:
        raise Fv3LmError(lib.err())


ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, _dp, C.c_int)


def set_allreduce_callback(lib, fn):
    """fn(buf: numpy view) must replace buf by its element-wise max over the ranks that hold faces (tracer_2d's
    mp_reduce_max of the per-level Courant numbers, fv_tracer2d_tlm.F90:1306).  Not needed with one rank."""
    def tramp(user, buf, n):
        fn(np.ctypeslib.as_array(buf, shape=(n,)))
    cb = ALLREDUCE_FN(tramp)
    lib._allreduce_cb = cb
    lib.L.fv3lm_set_allreduce_callback.argtypes = [ALLREDUCE_FN, C.c_void_p]
    lib.L.fv3lm_set_allreduce_callback(cb, None)


def set_transport_callback(lib, fn):
    """fn(peers, sendbufs, recvbufs): lists of numpy views (host memory in the emulation build).  Test transports (gloo)."""
    def tramp(user, npeers, peers, sb, sc, rb, rc):
        P = [peers[i] for i in range(npeers)]
        S = [np.ctypeslib.as_array(sb[i], shape=(sc[i],)) if sc[i] else np.zeros(0) for i in range(npeers)]
        R = [np.ctypeslib.as_array(rb[i], shape=(rc[i],)) if rc[i] else np.zeros(0) for i in range(npeers)]
        fn(P, S, R)
    cb = TRANSPORT_FN(tramp)
    lib._transport_cb = cb          # keep alive
    lib.L.fv3lm_set_transport_callback.argtypes = [TRANSPORT_FN, C.c_void_p]
    lib.L.fv3lm_set_transport_callback(cb, None)


def _ptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


class Dycore:
    """Device-resident dycore instance (one per GPU / MPI rank), cf. fv3jedi_lm_dynamics_type."""

    NL, TL, AD = 0, 1, 2

    def __init__(self, lib, dims, options, metrics, da_min, da_min_c, phis, ak, bk):
        self.lib, self.dims, self.options = lib, dims, options
        names = lib.metric_names()
        self.pj, self.pi = dims.ny + 7, dims.nx + 7
        arrs = []
        for n in names:
            a = np.ascontiguousarray(metrics[n], dtype=np.float64)
            assert a.shape == (dims.ntile, self.pj, self.pi), (n, a.shape)
            arrs.append(a)
        self._keep = arrs
        mp = (_dp * len(arrs))(*[_ptr(a) for a in arrs])
        self.h = C.c_void_p()
        phis = np.ascontiguousarray(phis, dtype=np.float64)
        ak = np.ascontiguousarray(ak, dtype=np.float64); bk = np.ascontiguousarray(bk, dtype=np.float64)
        rc = lib.L.fv3lm_create(C.byref(self.h), C.byref(dims), C.byref(options), mp, da_min, da_min_c,
                                _ptr(phis), _ptr(ak), _ptr(bk))
        if rc != 0:
            raise Fv3LmError(lib.err())

    def close(self):
        if self.h:
            self.lib.L.fv3lm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def levels(self, name):
        n = self.lib.L.fv3lm_field_levels(self.h, name.encode())
        if n < 0:
            raise Fv3LmError(self.lib.err())
        return n

    def shape(self, name):
        return (self.dims.ntile, self.levels(name), self.pj, self.pi)

    def put(self, name, arr, which=0):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        assert a.shape == self.shape(name), (name, a.shape, self.shape(name))
        if self.lib.L.fv3lm_field_put(self.h, name.encode(), which, _ptr(a)) != 0:
            raise Fv3LmError(self.lib.err())

    def get(self, name, which=0):
        a = np.empty(self.shape(name), dtype=np.float64)
        if self.lib.L.fv3lm_field_get(self.h, name.encode(), which, _ptr(a)) != 0:
            raise Fv3LmError(self.lib.err())
        return a

    def run_group(self, group, mode):
        if self.lib.L.fv3lm_run_group(self.h, group.encode(), mode) != 0:
            raise Fv3LmError(self.lib.err())

    def dyn_core(self, mode):
        if self.lib.L.fv3lm_dyn_core(self.h, mode) != 0:
            raise Fv3LmError(self.lib.err())

    def _chk(self, rc):
        if rc != 0:
            raise Fv3LmError(self.lib.err())

    def pressures(self, mode):
        self._chk(self.lib.L.fv3lm_pressures(self.h, mode))

    def tracer_2d(self, mode):
        self._chk(self.lib.L.fv3lm_tracer_2d(self.h, mode))

    def remap(self, mode, last_step):
        self._chk(self.lib.L.fv3lm_remap(self.h, mode, int(last_step)))

    def fv_dynamics(self, mode):
        self._chk(self.lib.L.fv3lm_fv_dynamics(self.h, mode))

    def step_tl(self):
        """fv3jedi_lm_dynamics_type%step_tl (DYN/fv3jedi_lm_dynamics_mod.F90:347-456), device part."""
        self._chk(self.lib.L.fv3lm_step_tl(self.h))

    def step_nl(self):
        self._chk(self.lib.L.fv3lm_step_nl(self.h))

    def step_ad(self):
        """%step_ad (DYN/fv3jedi_lm_dynamics_mod.F90:460-689): call after step_nl() (the FV_DYNAMICS_FWD
        role: nonlinear sweep storing the stage checkpoints)."""
        self._chk(self.lib.L.fv3lm_step_ad(self.h))

    # ---- Rayleigh damping of the upper layers (RAYLEIGH_SUPER, fv_dynamics_tlm.F90:1749-1899) ----
    def set_rayleigh(self, tau, rf_cutoff, c2l=None):
        """fv3lm_set_rayleigh: tau (days; 0 = off), rf_cutoff (Pa), c2l = a11 a12 a21 a22 as [ntile, 4, pj, pi] (None: NULL)."""
        ptr = None
        if c2l is not None:
            a = np.ascontiguousarray(c2l, dtype=np.float64)
            assert a.shape == (self.dims.ntile, 4, self.pj, self.pi), a.shape
            self._c2l = a
            ptr = _ptr(a)
        self.lib.L.fv3lm_set_rayleigh.argtypes = [C.c_void_p, C.c_double, C.c_double, _dp]
        self._chk(self.lib.L.fv3lm_set_rayleigh(self.h, float(tau), float(rf_cutoff), ptr))

    def rayleigh_profile(self):
        """-> (rf[npz], kmax) as the library computed them (rf = 0 below the cutoff)"""
        rf = np.zeros(self.dims.npz); kmax = C.c_int(0)
        self.lib.L.fv3lm_rayleigh_profile.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int)]
        self._chk(self.lib.L.fv3lm_rayleigh_profile(self.h, _ptr(rf), C.byref(kmax)))
        return rf, kmax.value

    def rayleigh(self, mode):
        """the damping on its own (tests): u v pt (w; non-hydrostatic: heated temperature in field "rf_pt"); adjoint after a NL call"""
        self.lib.L.fv3lm_rayleigh.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_rayleigh(self.h, mode))

    # ---- tracer damping of tracer_2d (nord_tr, trdm2 and their *_pert; fv_tracer2d_tlm.F90:1045-1111) ----
    def set_tracer_damping(self, nord_tr=0, trdm2=0.0, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1):
        """fv3lm_set_tracer_damping: after create, before a step or between complete steps; rebuilds the tracer program."""
        self.lib.L.fv3lm_set_tracer_damping.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int]
        self._chk(self.lib.L.fv3lm_set_tracer_damping(self.h, int(nord_tr), float(trdm2), int(nord_tr_pert), float(trdm2_pert), int(split_damp_tr)))

    def tracer_damping(self):
        """-> ((nord_tr, trdm2), (nord_tr_pert, trdm2_pert)): the effective trajectory and perturbation pairs"""
        n = (C.c_int * 2)(); d = (C.c_double * 2)()
        self.lib.L.fv3lm_tracer_damping.argtypes = [C.c_void_p, C.POINTER(C.c_int), _dp]
        self._chk(self.lib.L.fv3lm_tracer_damping(self.h, n, d))
        return (n[0], d[0]), (n[1], d[1])

    # ---- external-mode divergence damping of the acoustic step (flagstruct%d_ext; dyn_core_tlm.F90:1031-1060; csrc/dext.h) ----
    def set_external_damping(self, d_ext):
        """fv3lm_set_external_damping: after create, before a step or between complete steps; 0 = off (the default).  Going on or off
        rebuilds the acoustic program of a hydrostatic handle; a non-hydrostatic one remembers the value and launches nothing for it."""
        self.lib.L.fv3lm_set_external_damping.argtypes = [C.c_void_p, C.c_double]
        self._chk(self.lib.L.fv3lm_set_external_damping(self.h, float(d_ext)))

    def external_damping(self):
        """-> d_ext as set (0.0 on a handle that never called the setter)"""
        d = C.c_double(0.0)
        self.lib.L.fv3lm_external_damping.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(self.lib.L.fv3lm_external_damping(self.h, C.byref(d)))
        return d.value

    # ---- the trajectory's divergence-damping order after create (flagstruct%nord) ----
    def set_trajectory_damping_order(self, nord):
        """fv3lm_set_trajectory_damping_order: after create, before a step or between complete steps.  Resolves every level again and,
        when the order changed, rebuilds the acoustic program.  A non-hydrostatic handle reaches nord 2 and 3 only this way."""
        self.lib.L.fv3lm_set_trajectory_damping_order.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_set_trajectory_damping_order(self.h, int(nord)))

    def trajectory_damping_order(self):
        """-> the trajectory's nord as in force"""
        n = C.c_int(-1)
        self.lib.L.fv3lm_trajectory_damping_order.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self._chk(self.lib.L.fv3lm_trajectory_damping_order(self.h, C.byref(n)))
        return n.value

    # ---- linearised boundary-layer turbulence (fv3jedi_lm_turbulence_mod.F90; csrc/turbulence.h), compact arrays [ntile, npz, ny, nx] ----
    def _compact(self, a, nk=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        want = (self.dims.ntile,) + ((nk,) if nk else ()) + (self.dims.ny, self.dims.nx)
        assert a.shape == want, (a.shape, want)
        return a

    def turbulence_create(self, nslots=1):
        """fv3lm_turbulence_create: nslots x (9 factor arrays + pk) on the device (one slot per trajectory time kept)"""
        self.lib.L.fv3lm_turbulence_create.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_turbulence_create(self.h, int(nslots)))

    def turbulence_set_diagonals(self, slot, diag):
        """diag: AKV BKV CKV AKS BKS CKS AKQ BKQ CKQ (lower, main, upper; before the LU factorisation), nine compact arrays or None.
        pk is taken from the resident trajectory delp at this call: call after traj_to_fv3, before step_tl / step_nl."""
        if diag is None or len(diag) != 9:
            raise Fv3LmError("turbulence_set_diagonals: nine arrays needed")
        keep = [None if a is None else self._compact(a, self.dims.npz) for a in diag]
        ptrs = (_dp * 9)(*[None if a is None else _ptr(a) for a in keep])
        self.lib.L.fv3lm_turbulence_set_diagonals.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp)]
        self._chk(self.lib.L.fv3lm_turbulence_set_diagonals(self.h, int(slot), ptrs))

    def turbulence_set_simple(self, slot, frocean):
        """BL_simp (blsimp.F90) on the device from the resident trajectory; frocean compact [ntile, ny, nx] (None: NULL)"""
        a = None if frocean is None else self._compact(frocean)
        self.lib.L.fv3lm_turbulence_set_simple.argtypes = [C.c_void_p, C.c_int, _dp]
        self._chk(self.lib.L.fv3lm_turbulence_set_simple(self.h, int(slot), None if a is None else _ptr(a)))

    def bl_default_params(self, kpblmin):
        """fv3lm_bl_default_params: the TURBPARAMS / TURBPARAMSI documented at bldriver.F90:100-127; KPBLMIN = count(PREF < 50000) is the caller's"""
        p = BlParams()
        self.lib.L.fv3lm_bl_default_params.argtypes = [C.POINTER(BlParams), C.c_int]
        self.lib.L.fv3lm_bl_default_params.restype = None
        self.lib.L.fv3lm_bl_default_params(C.byref(p), int(kpblmin))
        return p

    SFC_NAMES = ("FRLAND", "FROCEAN", "VARFLT", "ZPBL", "CM", "CT", "CQ", "USTAR", "BSTAR")
    RAW_NAMES = ("AKV", "BKV", "CKV", "AKS", "BKS", "CKS", "AKQ", "BKQ", "CKQ", "EKV", "FKV", "ZPBL", "CT")

    def turbulence_set_driver(self, slot, params, dt, sfc, qa=None, qb=None, cloud_mode=0, raw=False):
        """BL_DRIVER (bldriver.F90) on the device from the resident trajectory, then the factorisation.  sfc: the nine surface fields
        in the order of SFC_NAMES (a dict by these names or a sequence; an entry None: NULL), compact [ntile, ny, nx]; qa, qb: QI, QL
        (cloud_mode 0) or QLS, QCN (cloud_mode 1), compact [ntile, npz, ny, nx] or None.  raw=True -> dict by RAW_NAMES of what BL_DRIVER
        left before the factorisation."""
        if isinstance(sfc, dict):
            sfc = [sfc.get(n) for n in self.SFC_NAMES]
        ptrs = None
        if sfc is not None:
            if len(sfc) != 9:
                raise Fv3LmError("turbulence_set_driver: nine surface arrays needed")
            keep = [None if a is None else self._compact(a) for a in sfc]
            ptrs = (_dp * 9)(*[None if a is None else _ptr(a) for a in keep])
        q = [None if a is None else self._compact(a, self.dims.npz) for a in (qa, qb)]
        out, optrs = None, None
        if raw:
            shp = (self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx)
            out = {n: np.empty(shp if k < 11 else (shp[0],) + shp[2:]) for k, n in enumerate(self.RAW_NAMES)}
            optrs = (_dp * 13)(*[_ptr(out[n]) for n in self.RAW_NAMES])
        f = self.lib.L.fv3lm_turbulence_set_driver
        f.argtypes = [C.c_void_p, C.c_int, C.POINTER(BlParams), C.c_double, C.POINTER(_dp), _dp, _dp, C.c_int, C.POINTER(_dp)]
        self._chk(f(self.h, int(slot), None if params is None else C.byref(params), float(dt), ptrs, None if q[0] is None else _ptr(q[0]),
                    None if q[1] is None else _ptr(q[1]), int(cloud_mode), optrs))
        return out

    def turbulence(self, slot, mode):
        """the seven solves of a slot: NL on the trajectory, TL on the perturbation, AD the transposed sweeps on the adjoint"""
        self.lib.L.fv3lm_turbulence.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_turbulence(self.h, int(slot), int(mode)))

    def turbulence_get(self, slot):
        """-> [10, ntile, npz, ny, nx]: the LU factors in the order of turbulence_set_diagonals, then pk"""
        out = np.empty((10, self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx))
        ptrs = (_dp * 10)(*[_ptr(out[n]) for n in range(10)])
        self.lib.L.fv3lm_turbulence_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp)]
        self._chk(self.lib.L.fv3lm_turbulence_get(self.h, int(slot), ptrs))
        return out

    # ---- linearised RAS convection (physics/moist/convection.F90; csrc/convection.h), compact arrays [ntile, (npz,) ny, nx] ----
    SET_NAMES = ("PTT_C", "QVT_C", "CNV_DQLDT_C", "CNV_MFD_C", "CNV_PRC3_C", "CNV_UPDF_C")
    SRC_NAMES = ("CNV_DQLDT", "CNV_MFD", "CNV_PRC3", "CNV_UPDF")

    def ras_default_params(self, im):
        """fv3lm_ras_default_params: RASPARAMS of create :120-148; entry 23 follows imsize = 4 im"""
        p = RasParams()
        self.lib.L.fv3lm_ras_default_params.argtypes = [C.POINTER(RasParams), C.c_int]
        self.lib.L.fv3lm_ras_default_params.restype = None
        self.lib.L.fv3lm_ras_default_params(C.byref(p), int(im))
        return p

    def convection_create(self, nslots, params, do_phy_mst):
        """fv3lm_convection_create: the slots, the sources and the work spaces of one batch of columns; all device memory of the feature"""
        self.lib.L.fv3lm_convection_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(RasParams), C.c_int]
        self._chk(self.lib.L.fv3lm_convection_create(self.h, int(nslots), None if params is None else C.byref(params), int(do_phy_mst)))

    def convection_set(self, slot, ts, frland, kcbl):
        """the slot takes the resident trajectory u v pt(= T) delp q1 at this call; ts, frland, kcbl compact [ntile, ny, nx] (None: NULL)"""
        a = [None if x is None else self._compact(x) for x in (ts, frland, kcbl)]
        self.lib.L.fv3lm_convection_set.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        self._chk(self.lib.L.fv3lm_convection_set(self.h, int(slot), *[None if x is None else _ptr(x) for x in a]))

    def convection_get(self, slot, jac=True):
        """-> (dict by SET_NAMES [ntile, npz, ny, nx], doconvec [ntile, ny, nx] int32, jac2 [2, ntile, npz, ny, nx] or None)"""
        shp = (self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx)
        out = {n: np.empty(shp) for n in self.SET_NAMES}
        ptrs = (_dp * 6)(*[_ptr(out[n]) for n in self.SET_NAMES])
        dc = np.zeros((shp[0],) + shp[2:], dtype=np.int32)
        j2 = np.empty((2,) + shp) if jac else None
        self.lib.L.fv3lm_convection_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp), C.POINTER(C.c_int), _dp]
        self._chk(self.lib.L.fv3lm_convection_get(self.h, int(slot), ptrs, dc.ctypes.data_as(C.POINTER(C.c_int)), None if j2 is None else _ptr(j2)))
        return out, dc, j2

    def convection_sources(self, src=None):
        """src None: -> the four sources of the perturbation (dict by SRC_NAMES); src (dict or sequence, an entry None: NULL): put them"""
        self.lib.L.fv3lm_convection_sources.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp)]
        if src is None:
            shp = (self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx)
            out = {n: np.empty(shp) for n in self.SRC_NAMES}
            self._chk(self.lib.L.fv3lm_convection_sources(self.h, 0, (_dp * 4)(*[_ptr(out[n]) for n in self.SRC_NAMES])))
            return out
        if isinstance(src, dict):
            src = [src.get(n) for n in self.SRC_NAMES]
        keep = [None if a is None else self._compact(a, self.dims.npz) for a in src]
        self._chk(self.lib.L.fv3lm_convection_sources(self.h, 1, (_dp * 4)(*[None if a is None else _ptr(a) for a in keep])))

    def convection_table(self):
        """-> (the saturation table as it lies on the device [18301], the kernels' constants CP ALHL GRAV RGAS H2OMW AIRMW VIREPS P00 KAPPA)"""
        tbl, cst = np.empty(18301), np.empty(9)
        self.lib.L.fv3lm_convection_table.argtypes = [C.c_void_p, _dp, _dp]
        self._chk(self.lib.L.fv3lm_convection_table(self.h, _ptr(tbl), _ptr(cst)))
        return tbl, cst

    def convection(self, slot, mode):
        """RAS convection in the DOCONVEC columns of the slot: NL on the trajectory, TL on the perturbation, AD on the adjoint"""
        self.lib.L.fv3lm_convection.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_convection(self.h, int(slot), int(mode)))

    # ---- linearised cloud scheme (physics/moist/cloud.F90; csrc/cloud.h), compact arrays [ntile, (npz,) ny, nx] ----
    CLOUD_NAMES = ("th", "q", "QI_ls", "QL_ls", "QI_con", "QL_con", "CF_ls", "CF_con")
    FRAC_NAMES = ("ILSF", "ICNF", "LLSF", "LCNF")

    def cloud_default_params(self, im):
        """fv3lm_cloud_default_params: CLOUDPARAMS of create :151-211; entries 42 and 46 follow imsize = 4 im"""
        p = CloudParams()
        self.lib.L.fv3lm_cloud_default_params.argtypes = [C.POINTER(CloudParams), C.c_int]
        self.lib.L.fv3lm_cloud_default_params.restype = None
        self.lib.L.fv3lm_cloud_default_params(C.byref(p), int(im))
        return p

    def cloud_create(self, params, iqi, iql):
        """fv3lm_cloud_create: after convection_create; one cloud slot per convection slot; iqi, iql: the tracers of cloud ice and liquid"""
        self.lib.L.fv3lm_cloud_create.argtypes = [C.c_void_p, C.POINTER(CloudParams), C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_cloud_create(self.h, None if params is None else C.byref(params), int(iqi), int(iql)))

    def cloud_bind_cfcn(self, iqc):
        """fv3lm_cloud_bind_cfcn: after cloud_create, before the first cloud_set: cfcn is tracer iqc of the dycore (trajectory and
        perturbation), carried by the dynamics as the reference's fifth tracer; cloud_set then accepts cfcn=None"""
        self.lib.L.fv3lm_cloud_bind_cfcn.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_cloud_bind_cfcn(self.h, int(iqc)))

    def cloud_set(self, slot, qls, qcn, cfcn, khl, khu):
        """after convection_set of the same slot: QLS QCN cfcn [ntile, npz, ny, nx], khl khu [ntile, ny, nx] (None: NULL)"""
        a = [None if x is None else self._compact(x, self.dims.npz) for x in (qls, qcn, cfcn)] + [None if x is None else self._compact(x) for x in (khl, khu)]
        self.lib.L.fv3lm_cloud_set.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
        self._chk(self.lib.L.fv3lm_cloud_set(self.h, int(slot), *[None if x is None else _ptr(x) for x in a]))

    def cloud_get(self, slot, out=True, frac=True, pertmod=True):
        """-> (dict by CLOUD_NAMES, dict by FRAC_NAMES, pertmod int32), each [ntile, npz, ny, nx] or None where not asked for"""
        shp = (self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx)
        o = {n: np.empty(shp) for n in self.CLOUD_NAMES} if out else None
        f = {n: np.empty(shp) for n in self.FRAC_NAMES} if frac else None
        pm = np.zeros(shp, dtype=np.int32) if pertmod else None
        self.lib.L.fv3lm_cloud_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp), C.POINTER(_dp), C.POINTER(C.c_int)]
        self._chk(self.lib.L.fv3lm_cloud_get(self.h, int(slot), None if o is None else (_dp * 8)(*[_ptr(o[n]) for n in self.CLOUD_NAMES]),
                                             None if f is None else (_dp * 4)(*[_ptr(f[n]) for n in self.FRAC_NAMES]),
                                             None if pm is None else pm.ctypes.data_as(C.POINTER(C.c_int))))
        return o, f, pm

    def cloud_cfcn(self, cfcn=None, null=False):
        """cfcn None: -> the perturbation's convective cloud fraction [ntile, npz, ny, nx]; else put it (null: pass NULL)"""
        self.lib.L.fv3lm_cloud_cfcn.argtypes = [C.c_void_p, C.c_int, _dp]
        if null:
            self._chk(self.lib.L.fv3lm_cloud_cfcn(self.h, 1, None))
        if cfcn is None:
            out = np.empty((self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx))
            self._chk(self.lib.L.fv3lm_cloud_cfcn(self.h, 0, _ptr(out)))
            return out
        keep = self._compact(cfcn, self.dims.npz)
        self._chk(self.lib.L.fv3lm_cloud_cfcn(self.h, 1, _ptr(keep)))

    def cloud(self, slot, mode):
        """the cloud scheme in every column of the slot: NL writes the trajectory tracers iqi, iql; TL on the perturbation; AD on the adjoint"""
        self.lib.L.fv3lm_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_cloud(self.h, int(slot), int(mode)))

    # ---- the composed model step (src/fv3jedi_lm_mod.F90:161-187; csrc/model.h) over stored trajectory times ----
    def lm_create(self, nslots, do_dyn=1, do_phy_trb=1, do_phy_mst=1):
        """fv3lm_lm_create: nslots trajectory slots (u v pt delp q* (w delz) phis, whole padded planes) in one allocation; the flags are
        conf%do_dyn, do_phy_trb and do_phy_mst /= 0, each 0 or 1, checked against the created features at the step"""
        self.lib.L.fv3lm_lm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_lm_create(self.h, int(nslots), int(do_dyn), int(do_phy_trb), int(do_phy_mst)))

    def lm_traj_save(self, slot):
        """the resident trajectory, halos included, into the slot (after traj_to_fv3 and the physics sets of that time)"""
        self.lib.L.fv3lm_lm_traj_save.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_lm_traj_save(self.h, int(slot)))

    def lm_traj_load(self, slot):
        """the slot back: the handle is then as after traj_to_fv3 of the same host arrays; the perturbation is not touched"""
        self.lib.L.fv3lm_lm_traj_load.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.L.fv3lm_lm_traj_load(self.h, int(slot)))

    def lm_step(self, slot, mode):
        """one step of the whole linear model about the trajectory of the slot, on the resident perturbation.  TL: dynamics, convection,
        cloud, turbulence; AD: turbulence, cloud, convection, dynamics (forward + backward sweep); cfcn cleared before and after"""
        self.lib.L.fv3lm_lm_step.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.L.fv3lm_lm_step(self.h, int(slot), int(mode)))

    # ---- the host's boundary copies on the device (compact arrays [ntile, nk, ny, nx], no halo) ----
    def _cptrs(self, d, names, out=False):
        keep = []
        required = ["u", "v", "pt", "delp"] + ["q%d" % (m + 1) for m in range(self.dims.nq)] + ([] if self.options.hydrostatic else ["w", "delz"])
        missing = [n for n in required if n not in d or d[n] is None]
        if missing:
            raise Fv3LmError("boundary copy: missing array(s) %s" % ", ".join(missing))
        def one(n):
            if n not in d or d[n] is None:
                return None
            a = d[n] if out else np.ascontiguousarray(d[n], dtype=np.float64)
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], n
            keep.append(a)
            return a.ctypes.data_as(_dp)
        nq = self.dims.nq
        qarr = (_dp * max(1, nq))(*[one("q%d" % (m + 1)) for m in range(nq)])
        return [one(n) for n in names], qarr, keep

    def traj_to_fv3(self, d):
        """d: dict of compact arrays u v pt delp q1.. (w delz) and optionally phis [ntile, ny, nx] (traj_to_fv3, :717-807)"""
        (u, v, t, dp, w, dz, ph), q, keep = self._cptrs(d, ["u", "v", "pt", "delp", "w", "delz", "phis"])
        f = self.lib.L.fv3lm_traj_to_fv3
        f.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.POINTER(_dp), _dp, _dp, _dp]
        self._chk(f(self.h, u, v, t, dp, q, w, dz, ph))

    def pert_to_fv3(self, d):
        (u, v, t, dp, w, dz), q, keep = self._cptrs(d, ["u", "v", "pt", "delp", "w", "delz"])
        f = self.lib.L.fv3lm_pert_to_fv3
        f.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.POINTER(_dp), _dp, _dp]
        self._chk(f(self.h, u, v, t, dp, q, w, dz))

    def fv3_to_pert(self, names):
        shp = (self.dims.ntile, self.dims.npz, self.dims.ny, self.dims.nx)
        d = {n: np.empty(shp) for n in names}
        (u, v, t, dp, w, dz), q, keep = self._cptrs(d, ["u", "v", "pt", "delp", "w", "delz"], out=True)
        f = self.lib.L.fv3lm_fv3_to_pert
        f.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.POINTER(_dp), _dp, _dp]
        self._chk(f(self.h, u, v, t, dp, q, w, dz))
        return d

    def state_save(self):
        self.lib.L.fv3lm_state_save.argtypes = [C.c_void_p]
        self._chk(self.lib.L.fv3lm_state_save(self.h))

    def state_restore(self):
        self.lib.L.fv3lm_state_restore.argtypes = [C.c_void_p]
        self._chk(self.lib.L.fv3lm_state_restore(self.h))

    def profile_begin(self):
        self.lib.L.fv3lm_profile_begin.argtypes = [C.c_void_p]
        self.lib.L.fv3lm_profile_begin(self.h)

    def profile_end(self):
        """-> {kernel: (launches, total_ms, algorithmic_bytes)} measured with HIP events on the library stream."""
        self.lib.L.fv3lm_profile_end.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        buf = C.create_string_buffer(1 << 16)
        self.lib.L.fv3lm_profile_end(self.h, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            n, cnt, ms, by = line.split()
            out[n] = (int(float(cnt)), float(ms), float(by))
        return out

    def zero_work_adjoint(self):
        self.lib.L.fv3lm_zero_work_adjoint(self.h)

    def sync(self):
        self.lib.L.fv3lm_sync(self.h)

    def launch_count(self):
        return self.lib.L.fv3lm_launch_count(self.h)

    def tp2_launch_count(self):
        return self.lib.L.fv3lm_tp2_launch_count(self.h)

    # ---- face mode (dims.face = 1) -------------------------------------------------------
    def set_face_data(self, edge, ecorner):
        """a2b_ord4 edge weights [ntile,4,pj] and extrap_corner factors [ntile,4,3] (cube.cubed_sphere_metrics)."""
        e = np.ascontiguousarray(edge, dtype=np.float64); c = np.ascontiguousarray(ecorner, dtype=np.float64)
        assert e.shape == (self.dims.ntile, 4, self.pj) and c.shape == (self.dims.ntile, 4, 3)
        self.lib.L.fv3lm_set_face_data.argtypes = [C.c_void_p, _dp, _dp]
        self._chk(self.lib.L.fv3lm_set_face_data(self.h, _ptr(e), _ptr(c)))

    HALO_KINDS = {"cell": 0, "dvec": 1, "cvec": 2, "corner": 3, "dedge": 4}

    def set_exchange(self, kind, rows):
        """Exchange table of one kind (cube.exchange_table / cube.boundary_table), int32 [n,7]."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        assert r.ndim == 2 and r.shape[1] == 7
        self.lib.L.fv3lm_set_exchange.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
        self._chk(self.lib.L.fv3lm_set_exchange(self.h, self.HALO_KINDS[kind], r.ctypes.data_as(C.POINTER(C.c_int)), r.shape[0]))

    def set_exchange_split(self, kind, table, rank, world, ntiles=6, loopback=False):
        """Install one exchange kind for this rank's tiles: local rows + per-peer send/receive lists (cube.split_table)."""
        from . import cube
        local, peers, send, recv = cube.split_table(table, rank, world, ntiles, loopback)
        self.set_exchange(kind, local)
        ip = C.POINTER(C.c_int)
        pe = np.array(peers, dtype=np.int32)
        ns = np.array([send[p].shape[0] for p in peers], dtype=np.int32); nr = np.array([recv[p].shape[0] for p in peers], dtype=np.int32)
        sr = np.ascontiguousarray(np.concatenate([send[p] for p in peers], axis=0) if peers else np.zeros((0, 3), np.int32))
        rr = np.ascontiguousarray(np.concatenate([recv[p] for p in peers], axis=0) if peers else np.zeros((0, 4), np.int32))
        self.lib.L.fv3lm_set_exchange_remote.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, ip, ip, ip]
        P = lambda a: a.ctypes.data_as(ip)
        self._chk(self.lib.L.fv3lm_set_exchange_remote(self.h, self.HALO_KINDS[kind], len(peers), P(pe), P(ns), P(sr), P(nr), P(rr)))

    def halo(self, kind, name0, name1="", mode=0):
        self.lib.L.fv3lm_halo.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        self._chk(self.lib.L.fv3lm_halo(self.h, self.HALO_KINDS[kind], name0.encode(), name1.encode(), mode))

    def level_params(self, k):
        ip = (C.c_int * 10)(); rp = (C.c_double * 6)()
        if self.lib.L.fv3lm_level_params(self.h, k, ip, rp) != 0:
            raise Fv3LmError(self.lib.err())
        return list(ip), list(rp)
