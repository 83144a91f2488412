"""Host-side mirror of the reference's call surface for the per-step solve.

    solver = nlpsol('solver', 'ipopt', cfg, opts)                 # C6:345-346
    sol    = solver(x0=, p=, lbx=, ubx=, lbg=, ubg=)              # C6:432 ; sol['x'] (n_var x 1)
    t0, u0 = shift(T, t0, u)                                      # C6:160-169,450

(C6 = AllScripts/centralized_six_robots_implementation.py.)  The batched overloads take a
leading batch dimension and keep everything on the GPU as torch tensors.  torch is used for
device memory and streams only; all arithmetic happens in libnmpc_hip.so through its C ABI.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from .problem import ProblemConfig


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the NMPC solve has no CPU fallback")
    return torch


def shift(T, t0, u):
    """C6:160-169: t0 += T ; u0 = [u[1:]; u[-1]] (drop first row, duplicate last)."""
    u = np.asarray(u)
    u0 = np.concatenate((u[1:u.shape[0], 0:], u[u.shape[0] - 1:u.shape[0], 0:]), axis=0)
    return t0 + T, u0


def shift_states(X, N=None):
    """C6:465: X0 = [X[1:]; X[N-1]] — the appended row is row N-1 of the (N+1)-row array."""
    X = np.asarray(X)
    N = X.shape[0] - 1 if N is None else N
    return np.concatenate((X[1:], X[N - 1:N]), axis=0)


def cold_start(cfg: ProblemConfig, x0) -> np.ndarray:
    """C6:398-400,423: X0 = repmat(x0), u0 = 0, packed [vec(X); vec(U)]."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    return np.concatenate([np.tile(x0, cfg.N + 1), np.zeros(cfg.nu * cfg.N)])


def odometry_to_global(odom, init, device=None, wrap_2pi: bool = False):
    """Batched odometry callback of the scripts (C2:18-37): odom [n,4] = (x_r, y_r, q_z, q_w), init [n,3] = (x, y, th) of the
    robot's start frame -> pose [n,3] in the global frame (device tensor).  Runs nmpc_odometry_batch.
    wrap_2pi: the modify() of the scripts without collision rows (AS/mpc_online_casadi.py:24-33), yaw in [-pi,0) -> +2 pi."""
    torch = _torch()
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    o = torch.as_tensor(odom, dtype=torch.float64, device=dev).reshape(-1, 4).contiguous()
    i0 = torch.as_tensor(init, dtype=torch.float64, device=dev).reshape(-1, 3).contiguous()
    if o.shape[0] != i0.shape[0]:
        raise ValueError(f"odom has {o.shape[0]} rows, init {i0.shape[0]}")
    pose = torch.empty((o.shape[0], 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.nmpc_odometry_batch(o.shape[0], o.data_ptr(), i0.data_ptr(), pose.data_ptr(), int(bool(wrap_2pi)), torch.cuda.current_stream().cuda_stream), "nmpc_odometry_batch")
    return pose


def split_swarm(p, m: int):
    """Independent-robot mode (AS/mpc_online_casadi_tb3_1.py et al. run one 3-state NLP per robot):
    p [B, 6m] = [x0 (3m); xs (3m)] of B swarms -> p1 [B*m, 6] of B*m single-robot problems (robot-major inside a swarm).
    Solve those with a ProblemConfig(m=1) solver; merge_swarm() puts the single-robot plans back side by side."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 6 * m)
    B = p.shape[0]
    return np.concatenate([p[:, : 3 * m].reshape(B, m, 3), p[:, 3 * m:].reshape(B, m, 3)], axis=2).reshape(B * m, 6)


def merge_swarm(w1, m: int, N: int):
    """w1 [B*m, 3(N+1)+2N] single-robot solutions -> w [B, (3m)(N+1)+(2m)N] in the centralized packing (C6:339)."""
    w1 = np.asarray(w1, dtype=np.float64)
    B = w1.shape[0] // m
    X = w1[:, : 3 * (N + 1)].reshape(B, m, N + 1, 3).transpose(0, 2, 1, 3).reshape(B, -1)
    U = w1[:, 3 * (N + 1):].reshape(B, m, N, 2).transpose(0, 2, 1, 3).reshape(B, -1)
    return np.concatenate([X, U], axis=1)


class NmpcSolver:
    """The object nlpsol() returns.  Owns a device workspace sized for `max_batch` instances."""

    def __init__(self, cfg: ProblemConfig, max_batch: int = 1, device: Optional[int] = None, kernel: Optional[int] = None,
                 trace_instance: Optional[int] = None):
        """kernel: None / 0 = the library picks the solve kernel per batch size; 1 / 2 / 3 pins the HBM-resident / element-per-lane /
        column-per-lane (throughput shape) kernel, 4 / 5 the column kernel's latency shape with two / four wavefronts per instance
        (nmpc_options_t).  The library itself reads no environment variable; this host class does, for development: NMPC_KERNEL (its
        first character, '1'..'5'; anything else = 0) and NMPC_TRACE_INST supply the two options when the arguments are not given."""
        import os
        self.cfg = cfg
        self.torch = _torch()
        self.lib = _lib.load()
        self.device = self.torch.device("cuda", self.torch.cuda.current_device() if device is None else device)
        self._ccfg = cfg.to_c()
        self._h = C.c_void_p()
        self.max_batch = int(max_batch)
        with self.torch.cuda.device(self.device):
            kv = os.environ.get("NMPC_KERNEL", "")
            opts = _lib.COptions(kernel=int(kernel) if kernel is not None else (int(kv[:1]) if kv[:1] in ("1", "2", "3", "4", "5") else 0),
                                 trace_instance=int(trace_instance) if trace_instance is not None else int(os.environ.get("NMPC_TRACE_INST", "-1")))
            _lib.check(self.lib.nmpc_create_opts(C.byref(self._ccfg), self.max_batch, C.byref(opts), C.byref(self._h)), "nmpc_create_opts")
        self.n_var, self.n_g, self.n_p = cfg.n_var, cfg.n_g, cfg.n_p
        assert self.n_var == self.lib.nmpc_n_var(C.byref(self._ccfg)) and self.n_g == self.lib.nmpc_n_g(C.byref(self._ccfg))
        self._stats: Dict = {}
        self._bounds = cfg.bounds()

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self.lib.nmpc_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.nmpc_workspace_bytes(self._h))

    def kernel_for_batch(self, B: int, ordered: bool = False) -> int:
        """the solve kernel nmpc_solve_batch launches for a batch of B (ordered: with a dispatch-order hint): 3 / 4 column-per-lane in its
        throughput / latency shape (4 covers two and four wavefronts per instance), 2 element-per-lane, 1 HBM-resident (nmpc_query)"""
        return int(self.lib.nmpc_query(self._h, _lib.QUERY_KERNEL_FOR_ORDERED_BATCH if ordered else _lib.QUERY_KERNEL_FOR_BATCH, int(B)))

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, a, shape):
        t = self.torch.as_tensor(a, dtype=self.torch.float64, device=self.device).reshape(shape).contiguous()
        return t

    def _obstacles(self, obstacles, B):
        """The per-instance obstacle field of a call: [B, K, 3] (static, S = 1) or [B, N, K, 3] (entry k: the obstacles at the time of X_k, S = N),
        K = len(cfg.obstacles) > 0, (ox, oy, r) per obstacle -> (contiguous float64 device tensor [B, S, K, 3], S)."""
        K, N = len(self.cfg.obstacles), self.cfg.N
        if K == 0:
            raise ValueError("obstacles= needs a handle with obstacle rows: a config with K entries in `obstacles` (they are the default field)")
        o = self.torch.as_tensor(obstacles, dtype=self.torch.float64, device=self.device)
        if o.dim() == 3 and tuple(o.shape) == (B, K, 3):
            o = o.reshape(B, 1, K, 3)
        elif not (o.dim() == 4 and tuple(o.shape) in ((B, N, K, 3), (B, 1, K, 3))):      # [B, 1, K, 3]: the C ABI's S = 1
            raise ValueError(f"obstacles must have shape ({B}, {K}, 3) or ({B}, {N}, {K}, 3), got {tuple(o.shape)}")
        return o.contiguous(), int(o.shape[1])

    def _reference(self, reference, B):
        """The pose reference of a call: [B, n_x] (one row for the horizon, S = 1) or [B, N, n_x] (row k: the reference of X_k, S = N)
        -> (contiguous float64 device tensor [B, S, n_x], S)."""
        nx, N = self.cfg.nx, self.cfg.N
        r = self.torch.as_tensor(reference, dtype=self.torch.float64, device=self.device)
        if r.dim() == 2 and tuple(r.shape) == (B, nx):
            r = r.reshape(B, 1, nx)
        elif not (r.dim() == 3 and tuple(r.shape) in ((B, N, nx), (B, 1, nx))):      # [B, 1, n_x]: the C ABI's S = 1
            raise ValueError(f"reference must have shape ({B}, {nx}) or ({B}, {N}, {nx}), got {tuple(r.shape)}")
        return r.contiguous(), int(r.shape[1])

    def _duals(self, B):
        """the multiplier outputs of a *_duals call: dict(lam_g [B, n_g], lam_x [B, n_var], lam_p [B, n_p]) of device tensors and their nmpc_duals_t"""
        torch = self.torch
        t = dict(lam_g=torch.empty((B, self.n_g), dtype=torch.float64, device=self.device),
                 lam_x=torch.empty((B, self.n_var), dtype=torch.float64, device=self.device),
                 lam_p=torch.empty((B, self.n_p), dtype=torch.float64, device=self.device))
        return t, _lib.CDuals(t["lam_g"].data_ptr(), t["lam_x"].data_ptr(), t["lam_p"].data_ptr())

    def duals_supported(self) -> bool:
        """whether this handle returns multipliers (it runs on the column-per-lane kernel): nmpc_solve_batch_duals answers an empty batch"""
        return self.lib.nmpc_solve_batch_duals(self._h, 0, None, None, 0, None, None, None, None, None, None, None, None, None) == 0

    # ---- batched device API -----------------------------------------------------------------
    def _order(self, order, B):
        """a dispatch-order hint as the int32 device tensor the C ABI reads (None stays None)"""
        if order is None:
            return None
        od = self.torch.as_tensor(order, device=self.device).to(self.torch.int32).contiguous()
        if od.shape != (B,):
            raise ValueError(f"order must have shape ({B},)")
        return od

    def solve_batch(self, p, w0, want_fg: bool = False, order=None, obstacles=None, want_duals: bool = False, reference=None):
        """p [B, 2 n_x], w0 [B, n_var] (torch cuda / numpy) -> dict of torch cuda tensors.

        order: optional permutation of range(B) (dispatch-order hint, nmpc_solve_batch_ordered): workgroup g solves instance
        order[g]; put the instances expected to need the most iterations first.  Results are unaffected.
        obstacles: optional per-instance obstacle field (nmpc_solve_batch_obs), [B, K, 3] static or [B, N, K, 3] per stage (entry k: the
        obstacles at the time of X_k), K = len(cfg.obstacles); the config's coordinates are then not used.
        want_duals: also return the multipliers of the returned point, lam_g [B, n_g], lam_x [B, n_var], lam_p [B, n_p], in CasADi's layout
        and sign (nmpc_solve_batch_duals, include/nmpc.h); the other results do not depend on it.
        reference: optional pose reference of the cost (nmpc_solve_batch_ref: trajectory tracking), [B, n_x] or [B, N, n_x] (row k: where X_k
        should be); the xs half of p is then not read.  Composes with order, obstacles, want_duals and want_fg (f and g then come from
        eval_batch(reference=)).  Needs a handle on the column-per-lane kernel (duals_supported())."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w0 = self._dev(w0, (B, self.n_var))
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        rf = self._reference(reference, B) if reference is not None else None
        w = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device)
        obj = torch.empty(B, dtype=torch.float64, device=self.device)
        kkt = torch.empty(B, dtype=torch.float64, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        iters = torch.empty(B, dtype=torch.int32, device=self.device)
        lam = {}
        with torch.cuda.device(self.device):
            od = self._order(order, B)
            if rf is not None:
                cd = None
                if want_duals:
                    lam, cd = self._duals(B)
                _lib.check(self.lib.nmpc_solve_batch_ref(self._h, B, p.data_ptr(), rf[0].data_ptr(), rf[1], ob[0].data_ptr() if ob is not None else None,
                                                         ob[1] if ob is not None else 0, w0.data_ptr(), w.data_ptr(), obj.data_ptr(), status.data_ptr(),
                                                         iters.data_ptr(), kkt.data_ptr(), od.data_ptr() if od is not None else None,
                                                         C.byref(cd) if cd is not None else None, self._stream()), "nmpc_solve_batch_ref")
            elif want_duals:
                lam, cd = self._duals(B)
                _lib.check(self.lib.nmpc_solve_batch_duals(self._h, B, p.data_ptr(), ob[0].data_ptr() if ob is not None else None, ob[1] if ob is not None else 0,
                                                           w0.data_ptr(), w.data_ptr(), obj.data_ptr(), status.data_ptr(), iters.data_ptr(), kkt.data_ptr(),
                                                           od.data_ptr() if od is not None else None, C.byref(cd), self._stream()), "nmpc_solve_batch_duals")
            elif ob is not None:
                _lib.check(self.lib.nmpc_solve_batch_obs(self._h, B, p.data_ptr(), ob[0].data_ptr(), ob[1], w0.data_ptr(), w.data_ptr(), obj.data_ptr(),
                                                         status.data_ptr(), iters.data_ptr(), kkt.data_ptr(), od.data_ptr() if od is not None else None,
                                                         self._stream()), "nmpc_solve_batch_obs")
            elif od is None:
                _lib.check(self.lib.nmpc_solve_batch(self._h, B, p.data_ptr(), w0.data_ptr(), w.data_ptr(), obj.data_ptr(),
                                                     status.data_ptr(), iters.data_ptr(), kkt.data_ptr(), self._stream()), "nmpc_solve_batch")
            else:
                _lib.check(self.lib.nmpc_solve_batch_ordered(self._h, B, p.data_ptr(), w0.data_ptr(), w.data_ptr(), obj.data_ptr(), status.data_ptr(),
                                                             iters.data_ptr(), kkt.data_ptr(), od.data_ptr(), self._stream()), "nmpc_solve_batch_ordered")
        out = dict(x=w, f=obj, status=status, iters=iters, kkt=kkt, **lam)
        if want_fg:
            f, g = self.eval_batch(p, w, obstacles=ob[0] if ob is not None else None, reference=rf[0] if rf is not None else None)
            out["f"], out["g"] = f, g
        return out

    def step_batch(self, p, w, order=None, obstacles=None, want_duals: bool = False, reference=None):
        """One control period on the device (nmpc_step_batch): solve from the guess w, then IN PLACE w <- shifted solution and
        p[:, :n_x] <- x0 + T f(x0, u_0); `order` [B] int32 device tensor (in: dispatch order of this period, out: the order for the
        next one, sorted by this period's iteration counts, longest first) or None.  p and w must be contiguous float64 device
        tensors owned by the caller (they are modified).  Returns sol['x'] of this period and the per-instance outputs.
        obstacles: optional per-instance obstacle field of this period (nmpc_step_batch_obs), as in solve_batch.
        want_duals: also return lam_g, lam_x, lam_p of this period's solution (nmpc_step_batch_duals), as in solve_batch.
        reference: optional pose reference of this period's window (nmpc_step_batch_ref), as in solve_batch; it is not written: the caller
        supplies the next period's window of its path."""
        torch = self.torch
        B = p.shape[0]
        if not (torch.is_tensor(p) and torch.is_tensor(w) and p.is_cuda and w.is_cuda and p.dtype == torch.float64 and w.dtype == torch.float64
                and p.is_contiguous() and w.is_contiguous() and p.shape == (B, self.n_p) and w.shape == (B, self.n_var)):
            raise ValueError("step_batch works in place: p [B, n_p] and w [B, n_var] must be contiguous float64 device tensors")
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        if order is not None and not (torch.is_tensor(order) and order.is_cuda and order.dtype == torch.int32 and order.is_contiguous() and order.shape == (B,)):
            raise ValueError("order must be a contiguous int32 device tensor of shape (B,)")
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        x = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device)
        obj = torch.empty(B, dtype=torch.float64, device=self.device); kkt = torch.empty(B, dtype=torch.float64, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device); iters = torch.empty(B, dtype=torch.int32, device=self.device)
        rf = self._reference(reference, B) if reference is not None else None
        with torch.cuda.device(self.device):
            if rf is not None:
                lam, cd = self._duals(B) if want_duals else ({}, None)
                _lib.check(self.lib.nmpc_step_batch_ref(self._h, B, p.data_ptr(), w.data_ptr(), x.data_ptr(), rf[0].data_ptr(), rf[1],
                                                        ob[0].data_ptr() if ob is not None else None, ob[1] if ob is not None else 0, obj.data_ptr(),
                                                        status.data_ptr(), iters.data_ptr(), kkt.data_ptr(), order.data_ptr() if order is not None else None,
                                                        C.byref(cd) if cd is not None else None, self._stream()), "nmpc_step_batch_ref")
                return dict(x=x, f=obj, status=status, iters=iters, kkt=kkt, order=order, **lam)
            if want_duals:
                lam, cd = self._duals(B)
                _lib.check(self.lib.nmpc_step_batch_duals(self._h, B, p.data_ptr(), w.data_ptr(), x.data_ptr(), ob[0].data_ptr() if ob is not None else None,
                                                          ob[1] if ob is not None else 0, obj.data_ptr(), status.data_ptr(), iters.data_ptr(), kkt.data_ptr(),
                                                          order.data_ptr() if order is not None else None, C.byref(cd), self._stream()), "nmpc_step_batch_duals")
                return dict(x=x, f=obj, status=status, iters=iters, kkt=kkt, order=order, **lam)
            if ob is not None:
                _lib.check(self.lib.nmpc_step_batch_obs(self._h, B, p.data_ptr(), w.data_ptr(), x.data_ptr(), ob[0].data_ptr(), ob[1], obj.data_ptr(),
                                                        status.data_ptr(), iters.data_ptr(), kkt.data_ptr(),
                                                        order.data_ptr() if order is not None else None, self._stream()), "nmpc_step_batch_obs")
                return dict(x=x, f=obj, status=status, iters=iters, kkt=kkt, order=order)
            _lib.check(self.lib.nmpc_step_batch(self._h, B, p.data_ptr(), w.data_ptr(), x.data_ptr(), obj.data_ptr(), status.data_ptr(), iters.data_ptr(),
                                                kkt.data_ptr(), order.data_ptr() if order is not None else None, self._stream()), "nmpc_step_batch")
        return dict(x=x, f=obj, status=status, iters=iters, kkt=kkt, order=order)

    def eval_batch(self, p, w, obstacles=None, reference=None):
        """f [B] and g [B, n_g] at w (nmpc_eval_batch); obstacles: optional per-instance obstacle field (nmpc_eval_batch_obs), reference: optional
        pose reference of the cost (nmpc_eval_batch_ref), [B, n_x] or [B, N, n_x] (row k: where X_k should be); the xs half of p is then not used."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var))
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        f = torch.empty(B, dtype=torch.float64, device=self.device)
        g = torch.empty((B, self.n_g), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            if reference is not None:
                rf = self._reference(reference, B)
                _lib.check(self.lib.nmpc_eval_batch_ref(self._h, B, p.data_ptr(), w.data_ptr(), rf[0].data_ptr(), rf[1], ob[0].data_ptr() if ob is not None else None,
                                                        ob[1] if ob is not None else 0, f.data_ptr(), g.data_ptr(), self._stream()), "nmpc_eval_batch_ref")
                return f, g
            if ob is not None:
                _lib.check(self.lib.nmpc_eval_batch_obs(self._h, B, p.data_ptr(), w.data_ptr(), ob[0].data_ptr(), ob[1], f.data_ptr(), g.data_ptr(),
                                                        self._stream()), "nmpc_eval_batch_obs")
                return f, g
            _lib.check(self.lib.nmpc_eval_batch(self._h, B, p.data_ptr(), w.data_ptr(), f.data_ptr(), g.data_ptr(), self._stream()), "nmpc_eval_batch")
        return f, g

    def kkt_batch(self, p, w, lam_g, lam_x, obstacles=None, want_grad: bool = False, reference=None):
        """KKT residuals of (w, lam_g, lam_x) for B instances on the device (nmpc_kkt_batch): res [B, 6] = (stat, eq, ineq, bnd, compl, sign) as
        include/nmpc.h defines them, and with want_grad also grad_lag [B, n_var] = grad f + J' lam_g + lam_x.  The multipliers may be a solve's
        (want_duals=True) or any others; obstacles as in solve_batch, reference (nmpc_kkt_batch_ref) as in eval_batch.  Works on every handle."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var)); lam_g = self._dev(lam_g, (B, self.n_g)); lam_x = self._dev(lam_x, (B, self.n_var))
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        res = torch.empty((B, 6), dtype=torch.float64, device=self.device)
        grad = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device) if want_grad else None
        with torch.cuda.device(self.device):
            if reference is not None:
                rf = self._reference(reference, B)
                _lib.check(self.lib.nmpc_kkt_batch_ref(self._h, B, p.data_ptr(), rf[0].data_ptr(), rf[1], ob[0].data_ptr() if ob is not None else None,
                                                       ob[1] if ob is not None else 0, w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), res.data_ptr(),
                                                       grad.data_ptr() if want_grad else None, self._stream()), "nmpc_kkt_batch_ref")
                return (res, grad) if want_grad else res
            _lib.check(self.lib.nmpc_kkt_batch(self._h, B, p.data_ptr(), ob[0].data_ptr() if ob is not None else None, ob[1] if ob is not None else 0,
                                               w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), res.data_ptr(), grad.data_ptr() if want_grad else None,
                                               self._stream()), "nmpc_kkt_batch")
        return (res, grad) if want_grad else res

    def sens_batch(self, p, w, lam_g, lam_x, dp=None, gains=None, obstacles=None):
        """Plan sensitivities and feedback gains of (w, lam_g, lam_x) for B instances on the device (nmpc_sens_batch): the linearisation of the
        solver's barrier KKT system at that primal-dual point, as include/nmpc.h defines it — usually a solve's output with want_duals=True.
        dp [B, n_p] = [dx0; dxs]: also return dw [B, n_var], the first-order change of the plan (w + dw predicts the solve at p + dp).
        gains: None (no gains), 1 (G_0 = dU_0*/dx0 only, [B, 1, n_u, n_x]) or "N" / the horizon (G_k = dU_k/dX_k of every stage, [B, N, n_u, n_x]).
        obstacles as in solve_batch.  Returns dict(dw, gains, info): info [B] int32 is 0 on success, 1 where the point is no strict minimiser
        of its barrier problem, 2 where a row or bound with a positive multiplier has no slack; dw and gains of such an instance are zeros.
        Needs a handle that returns multipliers (duals_supported()); the solver(x0=, p=, ...) call surface is unchanged."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var)); lam_g = self._dev(lam_g, (B, self.n_g)); lam_x = self._dev(lam_x, (B, self.n_var))
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        if gains not in (None, 1, "N", self.cfg.N):
            raise ValueError(f'gains must be None, 1 or "N" (= {self.cfg.N}), got {gains!r}')
        S = 0 if gains is None else (1 if gains == 1 else self.cfg.N)
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        dp = self._dev(dp, (B, self.n_p)) if dp is not None else None
        dw = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device) if dp is not None else None
        G = torch.empty((B, S, self.cfg.nu, self.cfg.nx), dtype=torch.float64, device=self.device) if S else None
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nmpc_sens_batch(self._h, B, p.data_ptr(), ob[0].data_ptr() if ob is not None else None, ob[1] if ob is not None else 0,
                                                w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), dp.data_ptr() if dp is not None else None,
                                                dw.data_ptr() if dw is not None else None, G.data_ptr() if S else None, S if S else 1,
                                                info.data_ptr(), self._stream()), "nmpc_sens_batch")
        return dict(dw=dw, gains=G, info=info)

    def sens_adjoint_batch(self, p, w, lam_g, lam_x, wbar, obstacles=None, want_pbar: bool = True, want_obsbar: Optional[bool] = None):
        """Adjoint plan sensitivities of (w, lam_g, lam_x) for B instances on the device (nmpc_sens_adjoint_batch): for a cotangent wbar [B, n_var] of
        the plan — the gradient of a scalar l(w*) — one launch returns pbar [B, n_p] = (dw*/dp)' wbar (x0 half, then xs half) and, with a
        per-instance obstacle field, obsbar = (dw*/dobstacles)' wbar in the shape of `obstacles` ([B, K, 3]: summed over the stages that share the
        entry; [B, N, K, 3]: entry 0 is zero), by the linearisation sens_batch uses.  obstacles as in solve_batch; without it obsbar is None (the
        config's own field is no per-instance parameter).  want_pbar / want_obsbar switch an output off (None; the other keeps its bits).
        Returns dict(pbar, obsbar, info): info [B] int32 as in sens_batch; the outputs of an instance with info != 0 are zeros.
        Needs a handle that returns multipliers (duals_supported())."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var)); lam_g = self._dev(lam_g, (B, self.n_g)); lam_x = self._dev(lam_x, (B, self.n_var))
        wbar = self._dev(wbar, (B, self.n_var))
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        if want_obsbar is None:
            want_obsbar = ob is not None
        if want_obsbar and ob is None:
            raise ValueError("obsbar needs obstacles=: the config's own field is not a per-instance parameter")
        pbar = torch.empty((B, self.n_p), dtype=torch.float64, device=self.device) if want_pbar else None
        obsbar = torch.empty(tuple(ob[0].shape), dtype=torch.float64, device=self.device) if want_obsbar else None
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nmpc_sens_adjoint_batch(self._h, B, p.data_ptr(), ob[0].data_ptr() if ob is not None else None, ob[1] if ob is not None else 0,
                                                        w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), wbar.data_ptr(),
                                                        pbar.data_ptr() if want_pbar else None, obsbar.data_ptr() if want_obsbar else None,
                                                        info.data_ptr(), self._stream()), "nmpc_sens_adjoint_batch")
        if obsbar is not None and len(getattr(obstacles, "shape", np.shape(obstacles))) == 3:
            obsbar = obsbar.reshape(B, len(self.cfg.obstacles), 3)
        return dict(pbar=pbar, obsbar=obsbar, info=info)

    def sens_update_batch(self, p, w, lam_g, lam_x, dp=None, dobs=None, rhs=None, obstacles=None, want_alpha: bool = True, want_duals: bool = False):
        """The forward plan update of (w, lam_g, lam_x) for B instances on the device (nmpc_sens_update_batch), one launch: dw [B, n_var], the
        first-order change of the plan for dp [B, n_p] = [dx0; dxs], a change dobs of the per-instance obstacle field (the shape of `obstacles`,
        [B, K, 3] or [B, N, K, 3]) and a general linear term rhs [B, n_var], each None for zero; and alpha [B], the largest step in (0, 1] along
        (dw, dobs) that keeps every linearised slack non-negative (1.0 exactly when nothing limits it; None with want_alpha=False, dw keeps its
        bits).  By the linearisation sens_batch uses; obstacles as in solve_batch, and dobs needs it (the config's own field is no per-instance
        parameter).  Returns dict(dw, alpha, info): info [B] int32 as in sens_batch; an instance with info != 0 gets dw = 0 and alpha = 0.
        Nothing is clipped: w + step * dw with step <= alpha is the caller's (nmpc_amd.AdvancedStepController).
        want_duals=True (nmpc_sens_update_batch_duals: the same launch, then one more on its stream) adds the multiplier updates that go with dw,
        dlam_g [B, n_g] and dlam_x [B, n_var], and alpha_dual [B], the largest step in (0, 1] that keeps every multiplier's sign: (w + a dw,
        lam_g + a dlam_g, lam_x + a dlam_x) is a primal-dual point at the moved parameters, for kkt_batch and for the sens_* calls.  dw, alpha and
        info keep their bits; zeros and alpha_dual = 0 where info != 0.
        Needs a handle that returns multipliers (duals_supported())."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var)); lam_g = self._dev(lam_g, (B, self.n_g)); lam_x = self._dev(lam_x, (B, self.n_var))
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        if dobs is not None and ob is None:
            raise ValueError("dobs needs obstacles=: the config's own field is not a per-instance parameter")
        dp = self._dev(dp, (B, self.n_p)) if dp is not None else None
        rhs = self._dev(rhs, (B, self.n_var)) if rhs is not None else None
        if dobs is not None:
            if tuple(getattr(dobs, "shape", np.shape(dobs))) != tuple(getattr(obstacles, "shape", np.shape(obstacles))):
                raise ValueError("dobs must have the shape of obstacles")
            dobs = self._dev(dobs, tuple(ob[0].shape))
        dw = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device)
        alpha = torch.empty(B, dtype=torch.float64, device=self.device) if want_alpha else None
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if want_duals:
            dlam_g = torch.empty((B, self.n_g), dtype=torch.float64, device=self.device)
            dlam_x = torch.empty((B, self.n_var), dtype=torch.float64, device=self.device)
            alpha_dual = torch.empty(B, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nmpc_sens_update_batch_duals(self._h, B, p.data_ptr(), ptr(ob[0]) if ob is not None else None, ob[1] if ob is not None else 0,
                                                                 w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), ptr(dp), ptr(dobs), ptr(rhs), dw.data_ptr(),
                                                                 ptr(alpha), dlam_g.data_ptr(), dlam_x.data_ptr(), alpha_dual.data_ptr(), info.data_ptr(),
                                                                 self._stream()), "nmpc_sens_update_batch_duals")
            return dict(dw=dw, alpha=alpha, info=info, dlam_g=dlam_g, dlam_x=dlam_x, alpha_dual=alpha_dual)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nmpc_sens_update_batch(self._h, B, p.data_ptr(), ptr(ob[0]) if ob is not None else None, ob[1] if ob is not None else 0,
                                                       w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), ptr(dp), ptr(dobs), ptr(rhs), dw.data_ptr(), ptr(alpha),
                                                       info.data_ptr(), self._stream()), "nmpc_sens_update_batch")
        return dict(dw=dw, alpha=alpha, info=info)

    @property
    def sens_dirs_per_pass(self) -> int:
        """how many directions of sens_update_multi the handle's kernel carries through one pass of its stage recursion (nmpc_query)"""
        return int(self.lib.nmpc_query(self._h, _lib.QUERY_SENS_DIRS_PER_PASS, 0))

    def sens_update_multi(self, p, w, lam_g, lam_x, dp=None, dobs=None, rhs=None, obstacles=None, want_alpha: bool = True, want_duals: bool = False):
        """sens_update_batch for D directions at the same point of every instance, one launch (nmpc_sens_update_batch_multi): dp [B, D, n_p],
        dobs [B, D, *field shape] (the field shape of `obstacles`: K, 3 or N, K, 3) and rhs [B, D, n_var], each None for zero and at least one
        given; D, at most 64, is taken from whichever is given.  Returns dict(dw [B, D, n_var], alpha [B, D] | None, info [B]): slot d is what
        sens_update_batch returns for direction d, to rounding; its bits do not depend on D or on the slot.  info is one verdict per instance;
        with info != 0 all D slots get dw = 0 and alpha = 0.  The part of the recursion that depends on the point only is done once.
        want_duals=True (nmpc_sens_update_batch_multi_duals: the same launch, then one more on its stream) adds the multiplier updates of every
        direction, dlam_g [B, D, n_g], dlam_x [B, D, n_var], dlam_p [B, D, n_p] (the change of lam_p: x0 part = dlam_g[..., :n_x], xs part
        2 Q (sum_k dX_k - N dxs)) and alpha_dual [B, D], slot d what sens_update_batch(want_duals=True) returns for direction d, to rounding; dw,
        alpha and info keep their bits; zeros and alpha_dual = 0 where info != 0.
        Needs a handle that returns multipliers (duals_supported())."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var)); lam_g = self._dev(lam_g, (B, self.n_g)); lam_x = self._dev(lam_x, (B, self.n_var))
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        ob = self._obstacles(obstacles, B) if obstacles is not None else None
        if dobs is not None and ob is None:
            raise ValueError("dobs needs obstacles=: the config's own field is not a per-instance parameter")
        given = [a for a in (dp, dobs, rhs) if a is not None]
        if not given:
            raise ValueError("at least one of dp, dobs, rhs must be given: the number of directions is taken from it")
        shapes = [tuple(getattr(a, "shape", np.shape(a))) for a in given]
        if any(len(s) < 3 or s[0] != B or s[1] != shapes[0][1] for s in shapes):
            raise ValueError(f"dp, dobs and rhs must be [{B}, D, ...] with one D, got {shapes}")
        D = int(shapes[0][1])
        if not 1 <= D <= _lib.SENS_MAX_DIRS:
            raise ValueError(f"D = {D} directions: 1 .. {_lib.SENS_MAX_DIRS} per call")
        dp = self._dev(dp, (B, D, self.n_p)) if dp is not None else None
        rhs = self._dev(rhs, (B, D, self.n_var)) if rhs is not None else None
        if dobs is not None:
            fshape = tuple(getattr(obstacles, "shape", np.shape(obstacles)))[1:]
            if tuple(getattr(dobs, "shape", np.shape(dobs))) != (B, D) + fshape:
                raise ValueError("dobs must have the shape [B, D] + the field shape of obstacles")
            dobs = self._dev(dobs, (B, D) + tuple(ob[0].shape[1:]))
        dw = torch.empty((B, D, self.n_var), dtype=torch.float64, device=self.device)
        alpha = torch.empty((B, D), dtype=torch.float64, device=self.device) if want_alpha else None
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if want_duals:
            dlam_g = torch.empty((B, D, self.n_g), dtype=torch.float64, device=self.device)
            dlam_x = torch.empty((B, D, self.n_var), dtype=torch.float64, device=self.device)
            dlam_p = torch.empty((B, D, self.n_p), dtype=torch.float64, device=self.device)
            alpha_dual = torch.empty((B, D), dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.nmpc_sens_update_batch_multi_duals(self._h, B, D, p.data_ptr(), ptr(ob[0]) if ob is not None else None, ob[1] if ob is not None else 0,
                                                                       w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), ptr(dp), ptr(dobs), ptr(rhs), dw.data_ptr(),
                                                                       ptr(alpha), dlam_g.data_ptr(), dlam_x.data_ptr(), dlam_p.data_ptr(), alpha_dual.data_ptr(),
                                                                       info.data_ptr(), self._stream()), "nmpc_sens_update_batch_multi_duals")
            return dict(dw=dw, alpha=alpha, info=info, dlam_g=dlam_g, dlam_x=dlam_x, dlam_p=dlam_p, alpha_dual=alpha_dual)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nmpc_sens_update_batch_multi(self._h, B, D, p.data_ptr(), ptr(ob[0]) if ob is not None else None, ob[1] if ob is not None else 0,
                                                             w.data_ptr(), lam_g.data_ptr(), lam_x.data_ptr(), ptr(dp), ptr(dobs), ptr(rhs), dw.data_ptr(),
                                                             ptr(alpha), info.data_ptr(), self._stream()), "nmpc_sens_update_batch_multi")
        return dict(dw=dw, alpha=alpha, info=info)

    def plan_jacobian(self, p, w, lam_g, lam_x, obstacles=None, wrt: str = "p", want_duals: bool = False):
        """The Jacobian of the plan at (w, lam_g, lam_x) by the linearisation sens_batch uses, from unit directions through sens_update_multi.
        wrt="p": J [B, n_var, n_p] = dw*/dp (x0 columns, then xs columns), one launch.  wrt="obstacles": J [B, n_var, S K 3] = dw*/dobstacles,
        columns in the order of the flattened field of `obstacles` ([B, K, 3]: S = 1; [B, N, K, 3]: S = N, the columns of entry 0 are zero), in
        as many launches of at most 64 directions as that takes.  Returns dict(J, info): info [B] as in sens_batch; J of an instance with
        info != 0 is zeros.  want_duals=True adds the Jacobians of the multipliers from the same launches (sens_update_multi(want_duals=True)):
        J_lam_g [B, n_g, cols], J_lam_x [B, n_var, cols] and, for wrt="p", J_lam_p [B, n_p, n_p]."""
        torch = self.torch
        if wrt not in ("p", "obstacles"):
            raise ValueError(f'wrt must be "p" or "obstacles", got {wrt!r}')
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        cols = lambda t: t.transpose(1, 2).contiguous()
        if wrt == "p":
            eye = torch.eye(self.n_p, dtype=torch.float64, device=self.device).expand(B, self.n_p, self.n_p)
            r = self.sens_update_multi(p, w, lam_g, lam_x, dp=eye, obstacles=obstacles, want_alpha=False, want_duals=want_duals)
            out = dict(J=cols(r["dw"]), info=r["info"])
            if want_duals:
                out.update(J_lam_g=cols(r["dlam_g"]), J_lam_x=cols(r["dlam_x"]), J_lam_p=cols(r["dlam_p"]))
            return out
        if obstacles is None:
            raise ValueError('wrt="obstacles" needs obstacles=: the config\'s own field is not a per-instance parameter')
        fshape = tuple(getattr(obstacles, "shape", np.shape(obstacles)))[1:]
        n = int(np.prod(fshape))
        J = torch.empty((B, self.n_var, n), dtype=torch.float64, device=self.device)
        Jg = torch.empty((B, self.n_g, n), dtype=torch.float64, device=self.device) if want_duals else None
        Jx = torch.empty((B, self.n_var, n), dtype=torch.float64, device=self.device) if want_duals else None
        info = None
        for lo in range(0, n, _lib.SENS_MAX_DIRS):
            hi = min(n, lo + _lib.SENS_MAX_DIRS)
            unit = torch.zeros((hi - lo, n), dtype=torch.float64, device=self.device)
            unit[torch.arange(hi - lo, device=self.device), torch.arange(lo, hi, device=self.device)] = 1.0
            r = self.sens_update_multi(p, w, lam_g, lam_x, dobs=unit.reshape((1, hi - lo) + fshape).expand((B, hi - lo) + fshape), obstacles=obstacles, want_alpha=False,
                                       want_duals=want_duals)
            J[:, :, lo:hi] = r["dw"].transpose(1, 2)
            if want_duals:
                Jg[:, :, lo:hi] = r["dlam_g"].transpose(1, 2)
                Jx[:, :, lo:hi] = r["dlam_x"].transpose(1, 2)
            info = r["info"]
        out = dict(J=J, info=info)
        if want_duals:
            out.update(J_lam_g=Jg, J_lam_x=Jx)
        return out

    def shift_batch(self, p, w, plant: bool = True):
        """device warm-start shift (C6:160-169,460-465) and, if plant, x0 + T f(x0,u0) (casadi_test.py:17-26)."""
        torch = self.torch
        p = self._dev(p, (-1, self.n_p)); B = p.shape[0]
        w = self._dev(w, (B, self.n_var))
        wn = torch.empty_like(w)
        x0n = torch.empty((B, self.cfg.nx), dtype=torch.float64, device=self.device) if plant else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nmpc_shift_batch(self._h, B, p.data_ptr(), w.data_ptr(), wn.data_ptr(),
                                                 x0n.data_ptr() if plant else None, self._stream()), "nmpc_shift_batch")
        return wn, x0n

    # ---- the reference's single-instance keyword call (C6:432) ----------------------------------
    def __call__(self, x0=None, p=None, lbx=None, ubx=None, lbg=None, ubg=None, **kw):
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")
        if p is None or x0 is None:
            raise ValueError("x0 and p are required")
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        w0 = np.asarray(x0, dtype=np.float64).reshape(-1)
        if p.size != self.n_p:
            raise ValueError(f"p has {p.size} entries, expected {self.n_p}")
        if w0.size != self.n_var:
            raise ValueError(f"x0 has {w0.size} entries, expected {self.n_var}")
        # bounds are structural here: accept (n,1)/(1,n)/flat, and insist they are the configured ones
        for name, given, want in (("lbx", lbx, self._bounds[0]), ("ubx", ubx, self._bounds[1]),
                                  ("lbg", lbg, self._bounds[2]), ("ubg", ubg, self._bounds[3])):
            if given is None:
                continue
            g = np.asarray(given, dtype=np.float64).reshape(-1)
            if g.size != want.size:
                raise ValueError(f"{name} has {g.size} entries, expected {want.size}")
            if not np.array_equal(g, want):
                raise ValueError(f"{name} differs from the bounds of the configured problem; build a new config instead")
        duals = self.duals_supported()      # the handle's kernel has the multipliers (sol['lam_g'], sol['lam_x'], sol['lam_p']) or the keys are absent
        r = self.solve_batch(p[None, :], w0[None, :], want_fg=True, want_duals=duals)
        self.torch.cuda.synchronize(self.device)
        st = int(r["status"][0])
        self._stats = dict(return_status=_lib.STATUS_NAMES.get(st, str(st)), success=(st == 0), iter_count=int(r["iters"][0]),
                           kkt_error=float(r["kkt"][0]), status_code=st)
        sol = {"x": r["x"][0].cpu().numpy().reshape(-1, 1), "f": float(r["f"][0]), "g": r["g"][0].cpu().numpy().reshape(-1, 1)}
        if duals:
            sol.update({k: r[k][0].cpu().numpy().reshape(-1, 1) for k in ("lam_g", "lam_x", "lam_p")})
        return sol

    def stats(self) -> Dict:
        """CasADi's solver.stats(); the reference never reads it, non-convergence is reported here only."""
        return dict(self._stats)


def nlpsol(name: str, plugin: str, problem, opts: Optional[dict] = None, max_batch: int = 1) -> NmpcSolver:
    """Drop-in for casadi.nlpsol(name,'ipopt',nlp_prob,opts) (C6:345-346) with `problem` a ProblemConfig.

    Honoured keys of opts['ipopt']: max_iter, tol / acceptable_tol, mu_init; print_* are accepted and ignored."""
    if plugin != "ipopt":
        raise ValueError("only the 'ipopt' call surface of the reference is mirrored")
    if not isinstance(problem, ProblemConfig):
        raise TypeError("problem must be a ProblemConfig (the symbolic CasADi graph is replaced by its parameters)")
    ip = dict((opts or {}).get("ipopt", {}))
    cfg = ProblemConfig(**{**problem.__dict__})
    if "max_iter" in ip: cfg.max_iter = int(ip["max_iter"])
    if "tol" in ip: cfg.tol = float(ip["tol"])
    elif "acceptable_tol" in ip: cfg.tol = float(ip["acceptable_tol"])
    if "mu_init" in ip: cfg.mu_init = float(ip["mu_init"])
    return NmpcSolver(cfg, max_batch=max_batch)


class PipelinedSolver:
    """Several launches in flight: `depth` handles (one workspace each) on `depth` HIP streams, used round-robin.  A launch lasts as long as its longest
    solve, so towards its end most of the device idles; the next batch's launch on another stream fills it (bench.py `two_streams`: six
    robots, B = 4096, 277 k -> 445 k solves/s with identical results).  Not part of the reference's call surface: a host-side convenience over the
    stream-ordered C ABI.

        pipe = PipelinedSolver(cfg, max_batch=4096)
        pending = [pipe.solve_batch(p_k, w0_k) for p_k, w0_k in batches]      # returns at once; results are ordered on the slot's stream
        pipe.synchronize()                                                    # or: r["event"].synchronize() for one result
    """

    def __init__(self, cfg: ProblemConfig, max_batch: int = 1, depth: int = 2, **kw):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.solvers = [NmpcSolver(cfg, max_batch=max_batch, **kw) for _ in range(depth)]
        self.torch = self.solvers[0].torch
        self.device = self.solvers[0].device
        with self.torch.cuda.device(self.device):
            self.streams = [self.torch.cuda.Stream() for _ in range(depth)]
        self._next = 0

    def solve_batch(self, p, w0, **kw):
        """NmpcSolver.solve_batch on the next slot's stream.  The slot's stream first waits for the caller's current stream (the inputs may still be in
        production there); the result carries `event`, recorded on the slot's stream after the solve — wait on it (or call synchronize()) before reading."""
        torch = self.torch
        k = self._next
        self._next = (k + 1) % len(self.solvers)
        st = self.streams[k]
        sol = self.solvers[k]
        p = sol._dev(p, (-1, sol.n_p))                       # on the caller's stream (a host array is copied there)
        w0 = sol._dev(w0, (p.shape[0], sol.n_var))
        if kw.get("obstacles") is not None:
            kw["obstacles"] = sol._obstacles(kw["obstacles"], p.shape[0])[0]      # the field too: [B, S, K, 3] on the device
        if kw.get("reference") is not None:
            kw["reference"] = sol._reference(kw["reference"], p.shape[0])[0]      # and the pose reference: [B, S, n_x] on the device
        st.wait_stream(torch.cuda.current_stream(self.device))
        p.record_stream(st); w0.record_stream(st)            # the caller may drop its references at once: the allocator must not hand the inputs out again before the solve has read them
        if kw.get("obstacles") is not None:
            kw["obstacles"].record_stream(st)
        if kw.get("reference") is not None:
            kw["reference"].record_stream(st)
        with torch.cuda.stream(st):
            r = sol.solve_batch(p, w0, **kw)
            ev = torch.cuda.Event()
            ev.record(st)
        r["event"] = ev
        r["slot"] = k
        return r

    def synchronize(self):
        for st in self.streams:
            st.synchronize()
