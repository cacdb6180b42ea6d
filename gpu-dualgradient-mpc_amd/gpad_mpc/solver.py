"""Host-side mirror of the reference's GPAD interfaces, on top of libgpad.so.

* ``solve(z0, y0, ML, M, G, g, N, L, tol)`` -- the north-star entry surface (BASELINE.json),
  numpy in / numpy out (host memory) or torch device tensors (device memory, in place).
* ``acceldualgrad(H, f, A_i, b_i, Qx, Qu, n_u)`` -- the reference MATLAB function
  (Code/MATLAB/acceldualgrad.m:1) with the same arguments and return ``u = z(1:n_u)``;
  precompute as acceldualgrad.m:11,20-23, the 100-iteration loop on the GPU.
* ``GpadSolver`` -- a handle: ``setup`` once per plant (constant ML/G), ``run`` per state.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Dims, Stats, check


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _count_array(arr, field: str, entries: int):
    """A caller's host iters / codes array for gpad_stats_t: int32, C-contiguous, >= entries."""
    if not isinstance(arr, np.ndarray) or arr.dtype != np.int32 or not arr.flags["C_CONTIGUOUS"] \
            or arr.size < entries:
        raise ValueError(f"{field} must be a C-contiguous host int32 array with >= {entries} entries")
    return arr.ctypes.data_as(C.POINTER(C.c_int))


def _dtype_code(x) -> int:
    if _is_torch(x):
        import torch
        if x.dtype == torch.float64:
            return _lib.DTYPE_F64
        if x.dtype == torch.float32:
            return _lib.DTYPE_F32
        raise TypeError(f"unsupported torch dtype {x.dtype}")
    if x.dtype == np.float64:
        return _lib.DTYPE_F64
    if x.dtype == np.float32:
        return _lib.DTYPE_F32
    raise TypeError(f"unsupported dtype {x.dtype}")


def _ptr(x):
    if _is_torch(x):
        if not x.is_contiguous():
            raise ValueError("device tensors must be contiguous")
        return C.c_void_p(x.data_ptr())
    if not x.flags["C_CONTIGUOUS"]:
        raise ValueError("host arrays must be C-contiguous")
    return C.c_void_p(x.ctypes.data)


class GpadSolver:
    """One libgpad handle (device + HIP stream + packed matrices + workspaces)."""

    def __init__(self, device: int = 0, stream=None):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        if stream is None and self._torch_device_ready():
            # order the solve after torch's pending work on this device (0 = HIP null stream)
            import torch
            stream = torch.cuda.current_stream(device).cuda_stream
        check(self.lib.gpad_create(C.byref(self.h), device, C.c_void_p(stream or 0)), "gpad_create")
        self._device = device
        self.dims = None
        self._classes = 0  # K of a class binding (setup_classes), 0: none
        self._last_steps = 0  # steps of the last closed_loop, 0 after any other run (last_restarts' shape)

    def last_phases(self) -> dict:
        """The phases the last phased panel solve launched (include/gpad.h gpad_last_phases): ends,
        finisher thresholds, survivors after each phase, whether the shape's plan prior was followed,
        and the finisher takeover (the first phase whose input the finisher took, its start
        iteration; None when the panels ran the whole solve)."""
        cap = 64
        ends, fins, counts = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        prior = C.c_int(0)
        n = self.lib.gpad_last_phases(self.h, ends, fins, counts, cap, C.byref(prior))
        check(min(n, 0), "gpad_last_phases")
        e, f, c = list(ends[:n]), list(fins[:n]), list(counts[:n])
        take = None
        for ph in range(1, n):
            if f[ph] > 0 and c[ph - 1] <= f[ph]:
                take = dict(phase=ph, iteration=e[ph - 1], survivors=c[ph - 1])
                break
        return dict(ends=e, fins=f, counts=c, prior=bool(prior.value), takeover=take)

    @staticmethod
    def _torch_device_ready() -> bool:
        try:
            import torch
            return torch.cuda.is_available()
        except Exception:  # noqa: BLE001 - torch is optional for host-memory use
            return False

    def close(self):
        if self.h:
            self.lib.gpad_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, name, value: int = _lib.OPT_DEFAULT) -> None:
        """gpad_set_option: schedule / launch tuning (``name`` in _lib.OPTIONS or a GPAD_OPT_*
        code); never changes results.  ``value`` -1 restores the default.

        ``"restart"`` (_lib.SOLVE_OPTIONS) is set here too and does change results: R >= 1 turns on the
        adaptive restart of the momentum with a decision every R iterations (include/gpad.h
        GPAD_OPT_RESTART; 0, the default, is off), see ``last_restarts``."""
        if isinstance(name, str):
            code = _lib.SOLVE_OPTIONS[name] if name in _lib.SOLVE_OPTIONS else _lib.OPTIONS[name]
        else:
            code = int(name)
        check(self.lib.gpad_set_option(self.h, code, int(value)), f"gpad_set_option({name})")

    def set_options(self, **kw) -> None:
        for k, v in kw.items():
            self.set_option(k, v)

    def set_stream(self, stream) -> None:
        check(self.lib.gpad_set_stream(self.h, C.c_void_p(stream or 0)), "gpad_set_stream")

    def setup(self, ML, G, L: float, *, n: int, m: int, batch: int = 1, shared: bool = True,
              schedule: int = _lib.SCHEDULE_MATLAB, check_every: int = 10,
              kernel: int = _lib.KERNEL_AUTO, scaled: bool = False, tol_gap: float = 0.0) -> None:
        """Bind (ML, G, L) -- or (MGneg, GL, L) with ``scaled`` (reference data-file form).
        ``tol_gap``: e_V of test (B)'s gap term (acceldualgrad.m:13; 0 = the run's tol)."""
        mem = _lib.MEM_DEVICE if _is_torch(ML) else _lib.MEM_HOST
        if _is_torch(ML) and not ML.is_cuda:
            raise ValueError("torch inputs must live on the GPU (use numpy for host memory)")
        self.dims = Dims(n=n, m=m, batch=batch, shared=int(bool(shared)), dtype=_dtype_code(ML),
                         memory=mem, schedule=schedule, check_every=check_every, kernel=kernel,
                         tol_gap=float(tol_gap))
        fn = self.lib.gpad_setup_scaled if scaled else self.lib.gpad_setup
        check(fn(self.h, C.byref(self.dims), _ptr(ML), _ptr(G), float(L)), "gpad_setup")
        self._classes = 0

    def setup_classes(self, ML, G, L: float, class_of, *, n: int, m: int, batch: int | None = None,
                      schedule: int = _lib.SCHEDULE_MATLAB, check_every: int = 10,
                      kernel: int = _lib.KERNEL_AUTO, tol_gap: float = 0.0) -> None:
        """Bind a fleet of K plant classes (gpad_setup_classes): ML (K, n, m), G (K, m, n), one L, and
        ``class_of`` [batch] host ints in 0..K-1 (``batch`` defaults to its length).  Packs of one class
        are solved together as a shared-matrix sub-batch, each class on the engine its own size picks;
        every array of ``run`` / ``run_state`` / ``closed_loop`` stays in the caller's instance order and
        the results are bit for bit those of ``setup(..., shared=False)`` on the expanded fleet
        (``problems.expand_classes``).  A stacked ``setup_plant`` then takes one copy of every map per
        class.  A later ``setup`` / ``setup_flat`` ends the binding."""
        if ML.ndim != 3 or G.ndim != 3 or G.shape[0] != ML.shape[0]:
            raise ValueError("setup_classes: ML must be (K, n, m) and G (K, m, n)")
        co = np.ascontiguousarray(np.asarray(class_of).reshape(-1), np.int32)
        if batch is None:
            batch = co.size
        if co.size != batch:
            raise ValueError(f"setup_classes: class_of has {co.size} entries, batch is {batch}")
        mem = _lib.MEM_DEVICE if _is_torch(ML) else _lib.MEM_HOST
        if _is_torch(ML) and not ML.is_cuda:
            raise ValueError("torch inputs must live on the GPU (use numpy for host memory)")
        dims = Dims(n=n, m=m, batch=batch, shared=1, dtype=_dtype_code(ML), memory=mem, schedule=schedule,
                    check_every=check_every, kernel=kernel, tol_gap=float(tol_gap))
        self._classes = 0
        check(self.lib.gpad_setup_classes(self.h, C.byref(dims), int(ML.shape[0]),
                                          co.ctypes.data_as(C.POINTER(C.c_int)), _ptr(ML), _ptr(G), float(L)),
              "gpad_setup_classes")
        self.dims = dims
        self._classes = int(ML.shape[0])

    def set_class_loop_fused(self, on: bool) -> None:
        """gpad_class_loop_fused: after ``setup_classes``, run ``closed_loop`` as one launch over every class
        (reported kernel "loop_classes") where the shape meets the rules of the ``loop_panel`` option; any
        other call runs class by class as before.  Results are bit for bit the same either way.  Off by
        default; a later ``setup_classes`` / ``setup*`` clears it."""
        check(self.lib.gpad_class_loop_fused(self.h, 1 if on else 0), "gpad_class_loop_fused")

    def setup_flat(self, MGf, GLf, L: float, *, n_u: int, batch: int = 1,
                   schedule: int = _lib.SCHEDULE_MATLAB, check_every: int = 10,
                   kernel: int = _lib.KERNEL_AUTO, tol_gap: float = 0.0) -> None:
        """Bind the reference's flat battery data (seq_functions.cpp:5-43): MGf (N x m) flat
        sign-folded M_G, GLf (m x N) flat G_L; then ``run(..., scaled=True)`` with g_P, p_D.
        kernel=KERNEL_STREAM forces the LDS flat kernel (else the register-resident one when
        6N, n <= 208)."""
        Nh, m = MGf.shape
        mem = _lib.MEM_DEVICE if _is_torch(MGf) else _lib.MEM_HOST
        self.dims = Dims(n=n_u * Nh, m=m, batch=batch, shared=1, dtype=_lib.DTYPE_F32, memory=mem,
                         schedule=schedule, check_every=check_every, kernel=kernel, tol_gap=float(tol_gap))
        check(self.lib.gpad_setup_flat(self.h, C.byref(self.dims), int(n_u), _ptr(MGf), _ptr(GLf),
                                       float(L)), "gpad_setup_flat")
        self._classes = 0

    def setup_hessian(self, H) -> None:
        """gpad_setup_hessian: bind the QP Hessian (same dtype / memory kind as ``setup``) so
        tol > 0 runs also evaluate the value-function branches (acceldualgrad.m:73,76); None
        unbinds."""
        check(self.lib.gpad_setup_hessian(self.h, _ptr(H) if H is not None else None), "gpad_setup_hessian")

    def setup_infeasibility(self, zbound: float) -> None:
        """gpad_setup_infeasibility: bind ``zbound`` = R > 0, a bound on |z|_inf over the feasible set
        (``problems.battery_zbound``), so tol > 0 runs end an infeasible solve early with code
        ``_lib.CODE_INFEASIBLE`` once its dual iterate certifies that no z of the box meets G z <= g
        (check it with ``farkas_margin``); 0 unbinds, as does every ``setup*``.  With a bound in force the
        solves run on the f32 T-wave panels (shared matrices, n, m <= 256) or else the stream kernel, the
        ``loop_panel`` option and the fused class loop keep their one-launch loops, and ``loop_async`` falls
        back to lockstep unless ``set_infeasibility_loop_async`` is on.  ``set_infeasibility_resident`` lets the
        resident kernel carry the certificate."""
        check(self.lib.gpad_setup_infeasibility(self.h, float(zbound)), "gpad_setup_infeasibility")

    def set_infeasibility_resident(self, on: bool) -> None:
        """gpad_infeasibility_resident: with a bound in force (``setup_infeasibility``, tol > 0) the f32 resident
        kernel carries the certificate where it applies (n, m <= 208): ``kernel=KERNEL_RESIDENT`` runs instead of
        raising, and AUTO takes the resident kernel where it takes it without a bound -- distinct matrices, or
        shared ones with batch <= 4 per CU -- lockstep loops and class bindings included (reported kernel
        "resident").  Results are bit for bit the same.  Off by default; a handle setting like an option: it
        survives ``setup*`` and unbinding, and a class binding forwards it to every class."""
        check(self.lib.gpad_infeasibility_resident(self.h, 1 if on else 0), "gpad_infeasibility_resident")

    def set_infeasibility_loop_async(self, on: bool) -> None:
        """gpad_infeasibility_loop_async: with a bound in force (``setup_infeasibility``, tol > 0) the ``loop_async``
        option keeps its one-launch loop (reported kernel "loop") on kernel variants that carry the certificate:
        a pack whose solve ends with code 5 applies u = z*[0:nu] and steps on like any other.  Results are bit for
        bit the lockstep loop's.  Every other condition of ``loop_async`` stands (f32, n, m <= 208, nx + ns <= 64,
        no forced PANEL / STREAM, no caller schedule tables); what it does not take falls back to lockstep as
        before.  Off by default and separate from ``set_infeasibility_resident``; a handle setting like an option:
        it survives ``setup*`` and unbinding, and a class binding forwards it to every class."""
        check(self.lib.gpad_infeasibility_loop_async(self.h, 1 if on else 0), "gpad_infeasibility_loop_async")

    def run(self, z, y, M, g, N: int, tol: float = 0.0, *, stats: bool = True, iters=None,
            scaled: bool = False, theta=None, beta=None, codes=None):
        """Run GPAD in place on z [batch][n] / y [batch][m].  Returns a dict of stats, or None
        when ``stats`` is False and the inputs are device tensors (asynchronous launch)."""
        st = Stats()
        nb = max(1, self.dims.batch if self.dims else 1)
        if iters is not None:
            st.iters = _count_array(iters, "iters", nb)
        if codes is not None:  # per-instance termination codes 0..5 (host int32 [batch])
            st.codes = _count_array(codes, "codes", nb)
        want = stats or not _is_torch(z)
        self._last_steps = 0
        for tab in (theta, beta):  # host tables whatever the memory kind (include/gpad.h)
            if tab is not None and (_is_torch(tab) or not isinstance(tab, np.ndarray)):
                raise TypeError("theta/beta must be host numpy arrays (include/gpad.h gpad_run_scaled)")
        if scaled:
            rc = self.lib.gpad_run_scaled(self.h, _ptr(z), _ptr(y), _ptr(M), _ptr(g), int(N),
                                          float(tol), _ptr(theta) if theta is not None else None,
                                          _ptr(beta) if beta is not None else None,
                                          C.byref(st) if want else None)
        else:
            rc = self.lib.gpad_run(self.h, _ptr(z), _ptr(y), _ptr(M), _ptr(g), int(N), float(tol),
                                   C.byref(st) if want else None)
        check(rc, "gpad_run")
        if not want:
            return None
        return self._stats_dict(st)

    def last_stats(self, iters=None, codes=None) -> dict:
        st = Stats()
        if iters is not None:
            st.iters = _count_array(iters, "iters", max(1, self.dims.batch if self.dims else 1))
        if codes is not None:
            st.codes = _count_array(codes, "codes", max(1, self.dims.batch if self.dims else 1))
        check(self.lib.gpad_last_stats(self.h, C.byref(st)), "gpad_last_stats")
        return self._stats_dict(st)

    def last_restarts(self):
        """Restarts of every solve of the last run (gpad_last_restarts): int32 [batch], or [steps][batch]
        after ``closed_loop``; zeros when that run had ``restart`` off or before any run."""
        batch = max(1, self.dims.batch if self.dims else 1)
        steps = self._last_steps
        buf = (C.c_int * (batch * max(1, steps)))()
        n = self.lib.gpad_last_restarts(self.h, buf, len(buf))
        check(min(n, 0), "gpad_last_restarts")
        out = np.zeros(len(buf), np.int32)
        out[:n] = buf[:n]
        return out.reshape(steps, batch) if steps else out

    def phase_plan(self) -> dict:
        """The phase plan the next phased panel solve follows (include/gpad.h gpad_phase_plan):
        phase ends, finisher thresholds, modelled time; empty lists = the default schedule."""
        cap = 64
        ends = (C.c_int * cap)()
        fins = (C.c_int * cap)()
        cost = C.c_double(0.0)
        n = self.lib.gpad_phase_plan(self.h, ends, fins, cap, C.byref(cost))
        check(min(n, 0), "gpad_phase_plan")
        return dict(ends=list(ends[:n]), fins=list(fins[:n]), cost_us=cost.value)

    def phase_counts(self) -> list:
        """Survivors after each phase of the last phased panel solve (gpad_phase_counts); trailing
        zeros trimmed."""
        cap = 64
        buf = (C.c_int * cap)()
        n = self.lib.gpad_phase_counts(self.h, buf, cap)
        check(min(n, 0), "gpad_phase_counts")
        out = list(buf[:n])
        while out and out[-1] == 0:
            out.pop()
        return out

    @staticmethod
    def plan_phases(iters, n: int, m: int, N: int, check_every: int = 10, num_cus: int = 256) -> dict:
        """gpad_plan_phases: the phase plan the panel solver would make from these per-instance
        iteration counts (host-only; runs without a GPU)."""
        L = _lib.load()
        it = np.ascontiguousarray(iters, np.int32)
        cap = 64
        ends = (C.c_int * cap)()
        fins = (C.c_int * cap)()
        cost = C.c_double(0.0)
        k = L.gpad_plan_phases(it.ctypes.data, it.size, n, m, N, check_every, num_cus, ends, fins, cap,
                               C.byref(cost))
        check(min(k, 0), "gpad_plan_phases")
        return dict(ends=list(ends[:k]), fins=list(fins[:k]), cost_us=cost.value)

    @staticmethod
    def _stats_dict(st: Stats) -> dict:
        return dict(iterations=st.iterations, converged=st.converged,
                    total_iterations=st.total_iterations, kernel=_lib.KERNEL_NAMES.get(st.kernel),
                    kernel_ms=st.kernel_ms, tol_floor=st.tol_floor,
                    below_tol_floor=bool(st.flags & _lib.FLAG_TOL_FLOOR),
                    nonfinite_g=bool(st.flags & _lib.FLAG_NONFINITE_G))

    def sync(self) -> None:
        check(self.lib.gpad_sync(self.h), "gpad_sync")

    # ---- per-state QP data / closed loop (gpad.m:79-95; include/gpad.h gpad_setup_plant) ---
    def accumulate_iterations(self, acc) -> None:
        """Enqueue acc += sum of the last run's per-instance iteration counts (acc: a 1-element
        int64 device tensor on this handle's device); no host synchronisation."""
        import torch
        if not (_is_torch(acc) and acc.is_cuda and acc.dtype == torch.int64 and acc.numel() >= 1):
            raise TypeError("acc must be an int64 CUDA tensor with at least one element")
        if self._device is not None and acc.device.index != self._device:
            raise ValueError(f"acc lives on cuda:{acc.device.index}, the handle on cuda:{self._device}")
        check(self.lib.gpad_accumulate_iterations(self.h, _ptr(acc)), "gpad_accumulate_iterations")

    def precompute(self, H, A, f=None, *, shared: bool = True):
        """acceldualgrad.m:11,20-21 on the device in fp64 (gpad_precompute): returns
        (ML = inv(H) A', gP = inv(H) f' or None, L = ||H||_F^2).  shared: one H (n x n), A (m x n)
        and f [batch][n]; else H [batch][n][n], A [batch][m][n], f [batch][n].  numpy in ->
        numpy out; torch (device, float64) in -> torch out."""
        dev = _is_torch(H)
        n = H.shape[-1]
        m = A.shape[-2]
        batch = (f.shape[0] if f is not None and f.ndim == 2 else 1) if shared else H.shape[0]
        nmat = 1 if shared else batch
        if dev:
            import torch
            H = H.to(torch.float64).contiguous()
            A = A.to(torch.float64).contiguous()
            f = None if f is None else f.to(torch.float64).contiguous()
            ML = torch.empty((nmat, n, m) if not shared else (n, m), dtype=torch.float64, device=H.device)
            gP = None if f is None else torch.empty_like(f)
            L = torch.empty(nmat, dtype=torch.float64, device=H.device)
            mem = _lib.MEM_DEVICE
        else:
            H = np.ascontiguousarray(H, np.float64)
            A = np.ascontiguousarray(A, np.float64)
            f = None if f is None else np.ascontiguousarray(f, np.float64)
            ML = np.empty((nmat, n, m) if not shared else (n, m))
            gP = None if f is None else np.empty_like(f)
            L = np.empty(nmat)
            mem = _lib.MEM_HOST
        opt = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        check(self.lib.gpad_precompute(self.h, n, m, batch, 1 if shared else 0, mem, _ptr(H), _ptr(A), opt(f),
                                       _ptr(ML), opt(gP), _ptr(L)), "gpad_precompute")
        return ML, gP, (float(L[0]) if shared else L)

    def lipschitz(self, ML, G, *, shared: bool = True, rtol: float = 0.01):
        """gpad_lipschitz: an upper bound of lambda_max(G ML), the smallest L ``setup`` may be given, within a
        factor 1 + rtol of it for ML = inv(H) G' (include/gpad.h), in fp64 on the device.  shared: ML (n, m),
        G (m, n) -> float; else ML [batch][n][m], G [batch][m][n] -> L [batch] (a fleet on one setup passes
        ``L.max()``).  float32 or float64, numpy in -> numpy out; torch device tensors in -> torch out."""
        ML, G, n, m, batch = _lipschitz_operands(ML, G, shared)
        if _is_torch(ML):
            import torch
            L = torch.empty(batch, dtype=torch.float64, device=ML.device)
            mem = _lib.MEM_DEVICE
        else:
            L = np.empty(batch)
            mem = _lib.MEM_HOST
        check(self.lib.gpad_lipschitz(self.h, n, m, batch, 1 if shared else 0, _dtype_code(ML), mem, _ptr(ML), _ptr(G),
                                      float(rtol), _ptr(L)), "gpad_lipschitz")
        return float(L[0]) if shared else L

    def setup_plant(self, PM, Pg, *, M0=None, g0=None, A=None, B=None) -> None:
        """Bind M(x) = M0 + PM x, g(x) = g0 + Pg x and (optionally) x+ = A x + B u.
        Same dtype / memory kind as the preceding ``setup``.

        One plant for the batch: PM (n, nx), Pg (m, nx), M0 (n), g0 (m), A (nx, nx), B (nx, nu).
        A stacked PM (batch, n, nx) binds per-instance maps (gpad_setup_plant_batch): every array
        given must then carry the leading batch axis.  That serves a fleet of distinct plants
        (``setup(..., shared=False)``) and one controller against per-instance true plants
        (``shared=True``) alike.

        After ``setup_classes`` a stacked PM leads with K instead, one copy of every map given per class
        (gpad_setup_plant_classes), and a 2-d PM binds the same maps for every class."""
        stacked = PM.ndim == 3
        arrays = dict(PM=PM, Pg=Pg, M0=M0, g0=g0, A=A, B=B)
        if stacked:
            batch = PM.shape[0]
            if self._classes and batch != self._classes:
                raise ValueError(f"setup_plant: PM is stacked for {batch} classes, setup_classes bound {self._classes}")
            if not self._classes and self.dims is not None and batch != self.dims.batch:
                raise ValueError(f"setup_plant: PM is stacked for {batch} instances, the setup has {self.dims.batch}")
            for name, a in arrays.items():
                want = 2 if name in ("M0", "g0") else 3
                if a is not None and (a.ndim != want or a.shape[0] != batch):
                    raise ValueError(f"setup_plant: PM is stacked (batch = {batch}), so {name} must be "
                                     f"{want}-dimensional with the same leading batch axis")
        nx = PM.shape[-1]
        nu = 0 if B is None else B.shape[-1]
        opt = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        fn = "gpad_setup_plant" if not stacked else ("gpad_setup_plant_classes" if self._classes
                                                     else "gpad_setup_plant_batch")
        check(getattr(self.lib, fn)(self.h, nx, nu, _ptr(PM), opt(M0), _ptr(Pg), opt(g0), opt(A), opt(B)), fn)

    def setup_signals(self, SM=None, Sg=None, E=None, *, ns: int | None = None) -> None:
        """Bind exogenous signals s (ns) on top of the plant (gpad_setup_signals):
        M(x, s) = M0 + PM x + SM s, g(x, s) = g0 + Pg x + Sg s, x+ = A x + E s + B u.
        SM (n, ns), Sg (m, ns), E (nx, ns) -- each with a leading batch axis after a stacked
        ``setup_plant`` -- in the dtype / memory kind of ``setup``; None is a map of zeros.  ``ns`` is
        read from the maps given, so it is needed only when all three are None; ``ns=0`` unbinds.
        Then pass ``s=`` to ``run_state`` and ``signals=`` to ``closed_loop``."""
        given = [a for a in (SM, Sg, E) if a is not None]
        if ns is None:
            if not given:
                raise ValueError("setup_signals: give a map or ns")
            ns = given[0].shape[-1]
        if any(a.shape[-1] != ns for a in given):
            raise ValueError(f"setup_signals: every map needs {ns} columns")
        opt = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        check(self.lib.gpad_setup_signals(self.h, int(ns), opt(SM), opt(Sg), opt(E)), "gpad_setup_signals")

    def setup_class_signals(self, SM=None, Sg=None, E=None, *, ns: int | None = None) -> None:
        """``setup_signals`` after ``setup_classes`` and ``setup_plant`` (gpad_setup_class_signals).
        Stacked maps SM (K, n, ns), Sg (K, m, ns), E (K, nx, ns) bind one copy per class, instance b using
        copy class_of[b]; 2-d maps serve every class.  Either goes with a stacked or a plain plant.  None is
        a map of zeros; ``ns`` is read from the maps given (needed when all three are None); ``ns=0``
        unbinds, as does a later ``setup_plant`` / ``setup_classes`` / ``setup*``.  Then pass ``s=`` to
        ``run_state`` and ``signals=`` to ``closed_loop`` in the caller's instance order; results are bit
        for bit those of ``setup(..., shared=False)`` + ``setup_signals`` on the expanded fleet."""
        given = [a for a in (SM, Sg, E) if a is not None]
        if ns is None:
            if not given:
                raise ValueError("setup_class_signals: give a map or ns")
            ns = given[0].shape[-1]
        if any(a.shape[-1] != ns for a in given):
            raise ValueError(f"setup_class_signals: every map needs {ns} columns")
        if any(a.ndim not in (2, 3) or a.ndim != given[0].ndim for a in given):
            raise ValueError("setup_class_signals: the maps must be all 2-dimensional or all stacked (K, rows, ns)")
        stacked = bool(given) and given[0].ndim == 3
        if stacked and self._classes and any(a.shape[0] != self._classes for a in given):
            raise ValueError(f"setup_class_signals: stacked maps must lead with K = {self._classes}")
        opt = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        check(self.lib.gpad_setup_class_signals(self.h, int(ns), 1 if stacked else 0, opt(SM), opt(Sg), opt(E)),
              "gpad_setup_class_signals")

    def run_state(self, x, z, y, N: int, tol: float = 0.0, *, stats: bool = True, s=None):
        """GPAD for every instance's state x [batch][nx] (M(x), g(x) formed on the device); with
        signals bound (``setup_signals``), ``s`` [batch][ns] is required."""
        st = Stats()
        self._last_steps = 0
        want = stats or not _is_torch(z)
        if s is not None:
            check(self.lib.gpad_run_state_signals(self.h, _ptr(x), _ptr(s), _ptr(z), _ptr(y), int(N), float(tol),
                                                  C.byref(st) if want else None), "gpad_run_state_signals")
        else:
            check(self.lib.gpad_run_state(self.h, _ptr(x), _ptr(z), _ptr(y), int(N), float(tol),
                                          C.byref(st) if want else None), "gpad_run_state")
        return self._stats_dict(st) if want else None

    def closed_loop(self, x, z, y, steps: int, N: int, tol: float = 0.0, *, warm: bool = False,
                    xs=None, us=None, iters=None, codes=None, stats: bool = True, signals=None):
        """gpad.m:79-95 on the device: ``steps`` receding-horizon MPC steps for every instance.
        x [batch][nx] is advanced in place; xs [steps][batch][nx] / us [steps][batch][nu]
        receive the trajectories when given; ``iters`` / ``codes`` (host int32 [steps*batch]) the
        counts and termination codes.

        The steps run in lockstep by default.  After ``set_option("loop_async", 1)`` the whole loop
        is one launch in which an instance starts its next step as soon as its own solve ends
        (``kernel == "loop"`` in the stats); it applies to f32 setups, shared matrices or per-instance
        ones, no flat setup and no Hessian, n, m <= 208, kernel AUTO or RESIDENT, N >= 1, nx <= 64 and
        nu <= min(n, 64), with one plant or per-instance maps (``setup_plant``), and any other call
        runs the lockstep loop -- also a call with an infeasibility bound in force (``setup_infeasibility``,
        tol > 0), unless ``set_infeasibility_loop_async(True)``.  Results are bit-identical.

        ``set_option("loop_panel", 1)`` is the same one-launch loop for fleets on the MFMA panels
        (``kernel == "loop_panel"``): a panel column whose solve ends steps to its instance's next
        solve in place.  It is looked at first and applies to f32 setups with shared matrices, no
        flat setup and no Hessian, n, m <= 256, kernel AUTO or PANEL, N >= 1, tol <= 0 or N a
        multiple of check_every, nx (+ ns) <= 64 and nu <= min(n, 64); any other call goes on as
        without it.  Results are bit-identical.

        With signals bound (``setup_signals``), ``signals`` [steps][batch][ns] is required: step t
        uses signals[t] for its QP data and for the update from x_t to x_{t+1}.  The one-launch loop
        then needs nx + ns <= 64."""
        st = Stats()
        self._last_steps = int(steps)
        for arr, field in ((iters, "iters"), (codes, "codes")):
            if arr is not None:
                setattr(st, field, _count_array(arr, field, steps * max(1, self.dims.batch if self.dims else 1)))
        want = stats or iters is not None or codes is not None or not _is_torch(z)
        opt = lambda a: _ptr(a) if a is not None else None  # noqa: E731
        if signals is not None:
            check(self.lib.gpad_closed_loop_signals(self.h, _ptr(x), _ptr(z), _ptr(y), _ptr(signals), int(steps),
                                                    int(N), float(tol), int(bool(warm)), opt(xs), opt(us),
                                                    C.byref(st) if want else None), "gpad_closed_loop_signals")
        else:
            check(self.lib.gpad_closed_loop(self.h, _ptr(x), _ptr(z), _ptr(y), int(steps), int(N),
                                            float(tol), int(bool(warm)), opt(xs), opt(us),
                                            C.byref(st) if want else None), "gpad_closed_loop")
        return self._stats_dict(st) if want else None

    # ---- per-step entry points (device tensors; kernel_functions.h one-for-one) ----------
    def step1(self, y, ym1, w, beta: float):
        check(self.lib.gpad_step1_extrapolate(self.h, _ptr(y), _ptr(ym1), _ptr(w), float(beta),
                                              y.numel()), "gpad_step1")

    def step2(self, MGneg, w, gP, zhat):
        n, m = MGneg.shape
        check(self.lib.gpad_step2_primal(self.h, _ptr(MGneg), _ptr(w), _ptr(gP), _ptr(zhat), n, m),
              "gpad_step2")

    def step2_flat(self, MGf, w, gP, zhat, n_u: int):
        """StepTwoGPADFlatSequential (seq_functions.cpp:5-20) on device tensors."""
        Nh, m = MGf.shape
        check(self.lib.gpad_step2_primal_flat(self.h, _ptr(MGf), _ptr(w), _ptr(gP), _ptr(zhat), Nh,
                                              n_u, m), "gpad_step2_flat")

    def step4_flat(self, GLf, yp1, w, pD, zhat, n_u: int):
        """StepFourGPADFlatSequential / StepFourGPADFlatParRows on device tensors."""
        m, Nh = GLf.shape
        check(self.lib.gpad_step4_project_flat(self.h, _ptr(GLf), _ptr(yp1), _ptr(w), _ptr(pD),
                                               _ptr(zhat), Nh, n_u, m), "gpad_step4_flat")

    def step3(self, theta: float, zm1, zhat, z):
        check(self.lib.gpad_step3_average(self.h, float(theta), _ptr(zm1), _ptr(zhat), _ptr(z),
                                          z.numel()), "gpad_step3")

    def step4(self, GL, yp1, w, pD, zhat):
        m, n = GL.shape
        check(self.lib.gpad_step4_project(self.h, _ptr(GL), _ptr(yp1), _ptr(w), _ptr(pD),
                                          _ptr(zhat), n, m), "gpad_step4")


class GpadGroup:
    """Several devices from one process (include/gpad.h gpad_group_*): contiguous instance shards,
    RCCL scatter/gather to devices[0] for device memory (peer copies when a device repeats)."""

    def __init__(self, devices):
        self.lib = _lib.load()
        self.devices = list(devices)
        arr = (C.c_int * len(self.devices))(*self.devices)
        self.g = C.c_void_p()
        check(self.lib.gpad_group_create(C.byref(self.g), len(self.devices), arr), "gpad_group_create")
        self.dims = None

    @property
    def transport(self) -> str:
        t = self.lib.gpad_group_transport(self.g)
        check(min(t, 0), "gpad_group_transport")
        return "rccl" if t == _lib.GROUP_RCCL else "peer"

    def close(self):
        if self.g:
            self.lib.gpad_group_destroy(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def setup(self, ML, G, L: float, *, n: int, m: int, batch: int, shared: bool = True,
              schedule: int = _lib.SCHEDULE_MATLAB, check_every: int = 10, kernel: int = _lib.KERNEL_AUTO,
              tol_gap: float = 0.0) -> None:
        mem = _lib.MEM_DEVICE if _is_torch(ML) else _lib.MEM_HOST
        self.dims = Dims(n=n, m=m, batch=batch, shared=int(bool(shared)), dtype=_dtype_code(ML), memory=mem,
                         schedule=schedule, check_every=check_every, kernel=kernel, tol_gap=float(tol_gap))
        check(self.lib.gpad_group_setup(self.g, C.byref(self.dims), _ptr(ML), _ptr(G), float(L)),
              "gpad_group_setup")

    def run(self, z, y, M, g, N: int, tol: float = 0.0, *, iters=None, codes=None) -> dict:
        st = Stats()
        nb = max(1, self.dims.batch if self.dims else 1)
        if iters is not None:
            st.iters = _count_array(iters, "iters", nb)
        if codes is not None:  # per-instance termination codes, [batch] in global order
            st.codes = _count_array(codes, "codes", nb)
        check(self.lib.gpad_group_run(self.g, _ptr(z), _ptr(y), _ptr(M), _ptr(g), int(N), float(tol),
                                      C.byref(st)), "gpad_group_run")
        return GpadSolver._stats_dict(st)


def farkas_margin(G, g, y, zbound: float) -> float:
    """gpad_farkas_margin: -(g'y) - zbound |G'y|_1 in fp64 on host arrays G (m, n), g (m), y (m) of one
    dtype (float32 or float64); -inf when y has a negative entry.  > 0 exactly when y proves that no z with
    |z|_inf <= zbound satisfies G z <= g.  Host only: runs without a GPU."""
    lib = _lib.load()
    G = np.ascontiguousarray(G)
    dt = G.dtype if G.dtype in (np.float32, np.float64) else np.float64
    G = np.ascontiguousarray(G, dt)
    g = np.ascontiguousarray(g, dt).reshape(-1)
    y = np.ascontiguousarray(y, dt).reshape(-1)
    m, n = G.shape
    if g.size != m or y.size != m:
        raise ValueError(f"farkas_margin: G is ({m}, {n}), so g and y need {m} entries")
    out = C.c_double(0.0)
    check(lib.gpad_farkas_margin(n, m, _dtype_code(G), _ptr(G), _ptr(g), _ptr(y), float(zbound), C.byref(out)),
          "gpad_farkas_margin")
    return out.value


def _lipschitz_operands(ML, G, shared: bool):
    """ML, G as contiguous arrays of one dtype (float32 kept, anything else float64) and (n, m, batch)."""
    if _is_torch(ML) != _is_torch(G):
        raise TypeError("lipschitz: ML and G must both be numpy arrays or both torch tensors")
    if _is_torch(ML):
        import torch
        dt = torch.float32 if ML.dtype == torch.float32 and G.dtype == torch.float32 else torch.float64
        ML, G = ML.to(dt).contiguous(), G.to(dt).contiguous()
    else:
        ML, G = np.asarray(ML), np.asarray(G)
        dt = np.float32 if ML.dtype == np.float32 and G.dtype == np.float32 else np.float64
        ML, G = np.ascontiguousarray(ML, dt), np.ascontiguousarray(G, dt)
    want = 2 if shared else 3
    if ML.ndim != want or G.ndim != want:
        raise ValueError(f"lipschitz: ML and G need {want} axes with shared={shared}")
    n, m = int(ML.shape[-2]), int(ML.shape[-1])
    if tuple(G.shape[-2:]) != (m, n) or (not shared and G.shape[0] != ML.shape[0]):
        raise ValueError(f"lipschitz: ML is {tuple(ML.shape)}, so G must be {tuple(ML.shape[:-2]) + (m, n)}")
    return ML, G, n, m, (1 if shared else int(ML.shape[0]))


def lipschitz_host(ML, G, *, shared: bool = True, rtol: float = 0.01):
    """gpad_lipschitz_host: ``GpadSolver.lipschitz`` in plain fp64 loops on host arrays -- no handle, no GPU.
    The check of the device kernel, and the way to a tight L on a box without one."""
    lib = _lib.load()
    ML, G, n, m, batch = _lipschitz_operands(np.asarray(ML), np.asarray(G), shared)
    L = np.empty(batch)
    check(lib.gpad_lipschitz_host(n, m, batch, 1 if shared else 0, _dtype_code(ML), _ptr(ML), _ptr(G), float(rtol),
                                  L.ctypes.data_as(C.POINTER(C.c_double))), "gpad_lipschitz_host")
    return float(L[0]) if shared else L


def schedule(N: int, kind: int = _lib.SCHEDULE_MATLAB):
    """theta[v], beta[v] (acceldualgrad.m:18,27,55-56) from the library's host routine."""
    lib = _lib.load()
    th = np.empty(max(N, 1), np.float64)
    be = np.empty(max(N, 1), np.float64)
    check(lib.gpad_schedule(N, kind, th.ctypes.data_as(C.POINTER(C.c_double)),
                            be.ctypes.data_as(C.POINTER(C.c_double))), "gpad_schedule")
    return th[:N], be[:N]


def solve(z0, y0, ML, M, G, g, N: int, L: float, tol: float = 0.0, *, shared: bool = True,
          schedule: int = _lib.SCHEDULE_MATLAB, check_every: int = 10,
          kernel: int = _lib.KERNEL_AUTO, device: int = 0, tol_gap: float = 0.0):
    """solve(z0, y0, ML, M, G, g, N, L, tol) -> (z*, y*, stats).

    Shapes: z0 (n,) or (batch, n); y0 (m,) or (batch, m); ML (n, m) or (batch, n, m); M like z0;
    G (m, n) or (batch, m, n); g like y0.  numpy inputs are copied (host memory); torch device
    tensors are updated in place."""
    torch_in = _is_torch(z0)
    if torch_in:
        z, y = z0, y0
    else:
        dt = np.float64 if np.asarray(ML).dtype == np.float64 else np.float32
        z = np.array(z0, dtype=dt, copy=True, order="C")
        y = np.array(y0, dtype=dt, copy=True, order="C")
        ML = np.ascontiguousarray(ML, dt)
        G = np.ascontiguousarray(G, dt)
        M = np.ascontiguousarray(M, dt)
        g = np.ascontiguousarray(g, dt)
    n, m = ML.shape[-2], ML.shape[-1]
    batch = z.shape[0] if z.ndim == 2 else 1
    shared = shared and ML.ndim == 2
    with GpadSolver(device) as s:
        s.setup(ML, G, L, n=n, m=m, batch=batch, shared=shared, schedule=schedule,
                check_every=check_every, kernel=kernel, tol_gap=tol_gap)
        st = s.run(z, y, M, g, N, tol)
    return z, y, st


def acceldualgrad(H, f, A_i, b_i, Qx=None, Qu=None, n_u: int = 1, num_iterations: int = 100,
                  dtype=np.float64, tol: float = 0.0):
    """Code/MATLAB/acceldualgrad.m:1 -- [u, z, y] with u = z(1:n_u) (:83).  Qx/Qu are accepted
    and unused, as in the reference.  Precompute (:11,20-23) on the host in fp64; the GPAD
    iterations run in libgpad on the GPU."""
    H = np.asarray(H, np.float64)
    A_i = np.asarray(A_i, np.float64)
    Hinv = np.linalg.inv(H)
    L = float(np.linalg.norm(H, "fro") ** 2)                    # acceldualgrad.m:11
    ML = Hinv @ A_i.T                                           # :20
    M = Hinv @ np.asarray(f, np.float64).reshape(-1)            # :21
    n, m = ML.shape
    z, y, _ = solve(np.zeros(n), np.zeros(m), ML.astype(dtype), M.astype(dtype), A_i.astype(dtype),
                    np.asarray(b_i, np.float64).astype(dtype), num_iterations, L, tol)
    return z[:n_u], z, y
