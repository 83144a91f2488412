"""Advanced-step NMPC among moving obstacles: solve ahead of time at the predicted state and field, then correct the plan with one cheap launch
when the measurement arrives.

prepare is one nmpc_solve_batch_duals launch, correct one nmpc_sens_update_batch launch on the solve's own primal-dual point (include/nmpc.h:
dw = S_p dp + S_o dobs and the step limit alpha).  The correction is applied over step = 1 where nothing limits it and tau * alpha elsewhere, so
that no linearised slack reaches zero; nothing is clipped.  torch carries the tensors; all arithmetic of the solve and of the update happens in
libnmpc_hip.so.
"""
from __future__ import annotations

from .solver import NmpcSolver


class AdvancedStepController:
    """ctl = AdvancedStepController(solver, tau=0.99); ctl.prepare(p_pred, w0, obstacles=obs_pred); out = ctl.correct(x0_measured, obstacles=obs_now)

    prepare(p_pred, w0, obstacles=None, **solve_kw) runs solve_batch(want_duals=True) and keeps (p, w, lam_g, lam_x, obstacles, status); it
    returns the solve's dict.  correct(x0_measured, xs=None, obstacles=None) takes dp = [x0_measured - x0_pred; xs - xs_pred] and
    dobs = obstacles - obstacles_pred (a missing argument: unchanged) through one sens_update_batch launch and returns
    dict(w, u0, step, alpha, info, corrected): step [B] is 1 where alpha == 1 and tau * alpha elsewhere, w = w_pred + step * dw where the solve's
    status and the update's verdict are both 0 and the prepared plan unchanged elsewhere (corrected [B] bool False; their count is
    .last['uncorrected']), u0 [B, n_u] the first control of w.  The controller changes no solver state and may be corrected any number of times
    per prepare.

    correct(..., update_duals=True) runs nmpc_sens_update_batch_duals: the multipliers move with the plan, so the corrected point can be
    certified (kkt_batch at the moved parameters) or linearised again (sens_*).  The step is then the smaller of the primal one and
    1 where alpha_dual == 1, tau * alpha_dual elsewhere — no multiplier changes sign either — and the dict gains lam_g, lam_x (moved by the
    same step; the prepared ones where corrected is False) and alpha_dual.
    correct(..., commit=True) implies update_duals and makes the corrected point the controller's base on the corrected instances:
    (p + step dp, obstacles + step dobs, w, lam_g, lam_x) replace the prepared ones there, the next correct() linearises at them and takes its
    dp and dobs relative to them; the other instances keep their base.  With both flags off nothing changes.
    correct_scenarios(...) is correct() for D scenarios in one launch; with update_duals=True every scenario keeps multipliers, and
    commit_scenario(d) makes one of them the base as correct(..., commit=True) would."""

    def __init__(self, solver: NmpcSolver, tau: float = 0.99):
        if not solver.duals_supported():
            raise RuntimeError("AdvancedStepController needs a handle that returns multipliers (the column-per-lane kernel): this one is pinned to kernel 1 or 2")
        if not 0.0 < tau <= 1.0:
            raise ValueError(f"tau must lie in (0, 1], got {tau!r}")
        self.solver = solver
        self.tau = float(tau)
        self.last = {}
        self._plan = None
        self._scenarios = None      # what the last correct_scenarios(update_duals=True) left for commit_scenario

    def prepare(self, p_pred, w0, obstacles=None, **solve_kw):
        s = self.solver
        torch = s.torch
        p = s._dev(p_pred, (-1, s.n_p))
        obs = None if obstacles is None else torch.as_tensor(obstacles, dtype=torch.float64, device=s.device)
        r = s.solve_batch(p, w0, obstacles=obs, want_duals=True, **solve_kw)
        self._plan = dict(p=p, w=r["x"], lam_g=r["lam_g"], lam_x=r["lam_x"], obstacles=obs, status=r["status"])
        self.last = dict(status=r["status"], iters=r["iters"], kkt=r["kkt"], f=r["f"])
        return r

    def correct(self, x0_measured, xs=None, obstacles=None, update_duals: bool = False, commit: bool = False):
        if self._plan is None:
            raise RuntimeError("correct() needs a prepared plan: call prepare() first")
        s, pl = self.solver, self._plan
        torch = s.torch
        nx, nu, N = s.cfg.nx, s.cfg.nu, s.cfg.N
        B = pl["p"].shape[0]
        duals = update_duals or commit
        dp = torch.zeros_like(pl["p"])
        dp[:, :nx] = s._dev(x0_measured, (B, nx)) - pl["p"][:, :nx]
        if xs is not None:
            dp[:, nx:] = s._dev(xs, (B, nx)) - pl["p"][:, nx:]
        dobs = None
        if obstacles is not None:
            if pl["obstacles"] is None:
                raise ValueError("obstacles= needs a plan prepared with obstacles=: the config's own field is not a per-instance parameter")
            dobs = torch.as_tensor(obstacles, dtype=torch.float64, device=s.device).reshape(pl["obstacles"].shape) - pl["obstacles"]
        out = s.sens_update_batch(pl["p"], pl["w"], pl["lam_g"], pl["lam_x"], dp=dp, dobs=dobs, obstacles=pl["obstacles"], want_duals=duals)
        alpha, info = out["alpha"], out["info"]
        step = torch.where(alpha == 1.0, alpha, self.tau * alpha)
        if duals:
            ad = out["alpha_dual"]
            step = torch.minimum(step, torch.where(ad == 1.0, ad, self.tau * ad))
        ok = (pl["status"] == 0) & (info == 0)
        w = torch.where(ok[:, None], pl["w"] + step[:, None] * out["dw"], pl["w"])
        self.last["info"] = info
        self.last["uncorrected"] = int((~ok).sum())
        uo = (N + 1) * nx
        res = dict(w=w, u0=w[:, uo: uo + nu], step=step, alpha=alpha, info=info, corrected=ok)
        if duals:
            res["lam_g"] = torch.where(ok[:, None], pl["lam_g"] + step[:, None] * out["dlam_g"], pl["lam_g"])
            res["lam_x"] = torch.where(ok[:, None], pl["lam_x"] + step[:, None] * out["dlam_x"], pl["lam_x"])
            res["alpha_dual"] = out["alpha_dual"]
        if commit:
            obs = pl["obstacles"]
            if dobs is not None:
                okf = ok.reshape((B,) + (1,) * (obs.dim() - 1))
                obs = torch.where(okf, obs + step.reshape(okf.shape) * dobs, obs)
            self._plan = dict(p=torch.where(ok[:, None], pl["p"] + step[:, None] * dp, pl["p"]), w=w, lam_g=res["lam_g"], lam_x=res["lam_x"],
                              obstacles=obs, status=pl["status"])
        return res

    def correct_scenarios(self, x0_candidates, xs=None, obstacles=None, update_duals: bool = False):
        """correct() for D scenarios of every instance in one sens_update_multi launch: x0_candidates [B, D, n_x], xs [B, D, n_x] or None
        (unchanged), obstacles [B, D] + the field shape of the prepared obstacles, or None (unchanged).  Returns dict(w [B, D, n_var],
        u0 [B, D, n_u], step [B, D], alpha [B, D], info [B], corrected [B]): scenario d by the rule of correct() — step is 1 where alpha == 1 and
        tau * alpha elsewhere, w = w_pred + step * dw where the solve's status and the update's verdict are both 0, the prepared plan in every
        scenario elsewhere.  .last['uncorrected'] counts the instances as correct() does.
        update_duals=True runs nmpc_sens_update_batch_multi_duals: every scenario's multipliers move with its plan by the rule of
        correct(update_duals=True) — the step is the smaller of the primal one and 1 where alpha_dual == 1, tau * alpha_dual elsewhere — and the
        dict gains lam_g [B, D, n_g], lam_x [B, D, n_var] (the prepared ones in every scenario where corrected is False) and alpha_dual [B, D].
        commit_scenario(d) then makes one of the scenarios the controller's base."""
        if self._plan is None:
            raise RuntimeError("correct_scenarios() needs a prepared plan: call prepare() first")
        s, pl = self.solver, self._plan
        torch = s.torch
        nx, nu, N = s.cfg.nx, s.cfg.nu, s.cfg.N
        B = pl["p"].shape[0]
        x0c = torch.as_tensor(x0_candidates, dtype=torch.float64, device=s.device)
        if x0c.dim() != 3 or x0c.shape[0] != B or x0c.shape[2] != nx:
            raise ValueError(f"x0_candidates must have shape ({B}, D, {nx}), got {tuple(x0c.shape)}")
        D = x0c.shape[1]
        dp = torch.zeros((B, D, 2 * nx), dtype=torch.float64, device=s.device)
        dp[:, :, :nx] = x0c - pl["p"][:, None, :nx]
        if xs is not None:
            dp[:, :, nx:] = s._dev(xs, (B, D, nx)) - pl["p"][:, None, nx:]
        dobs = None
        if obstacles is not None:
            if pl["obstacles"] is None:
                raise ValueError("obstacles= needs a plan prepared with obstacles=: the config's own field is not a per-instance parameter")
            fshape = tuple(pl["obstacles"].shape[1:])
            dobs = torch.as_tensor(obstacles, dtype=torch.float64, device=s.device).reshape((B, D) + fshape) - pl["obstacles"][:, None]
        if update_duals:
            out = s.sens_update_multi(pl["p"], pl["w"], pl["lam_g"], pl["lam_x"], dp=dp, dobs=dobs, obstacles=pl["obstacles"], want_duals=True)
        else:
            out = s.sens_update_multi(pl["p"], pl["w"], pl["lam_g"], pl["lam_x"], dp=dp, dobs=dobs, obstacles=pl["obstacles"])
        alpha, info = out["alpha"], out["info"]
        step = torch.where(alpha == 1.0, alpha, self.tau * alpha)
        if update_duals:
            ad = out["alpha_dual"]
            step = torch.minimum(step, torch.where(ad == 1.0, ad, self.tau * ad))
        ok = (pl["status"] == 0) & (info == 0)
        moved = lambda base, d: torch.where(ok[:, None, None], base[:, None, :] + step[:, :, None] * d, base[:, None, :].expand(B, D, base.shape[1]))
        w = moved(pl["w"], out["dw"])
        self.last["info"] = info
        self.last["uncorrected"] = int((~ok).sum())
        uo = (N + 1) * nx
        res = dict(w=w, u0=w[:, :, uo: uo + nu], step=step, alpha=alpha, info=info, corrected=ok)
        self._scenarios = None
        if update_duals:
            res["lam_g"] = moved(pl["lam_g"], out["dlam_g"])
            res["lam_x"] = moved(pl["lam_x"], out["dlam_x"])
            res["alpha_dual"] = out["alpha_dual"]
            self._scenarios = dict(plan=pl, dp=dp, dobs=dobs, step=step, ok=ok, w=w, lam_g=res["lam_g"], lam_x=res["lam_x"])
        return res

    def commit_scenario(self, d):
        """After correct_scenarios(update_duals=True): scenario d (an int, or [B] indices, one scenario per instance) becomes the controller's
        base on the corrected instances — (p + step dp, obstacles + step dobs, w, lam_g, lam_x) of that scenario replace the prepared ones there,
        exactly what correct(..., commit=True) on that scenario would have left; the other instances keep their base.  The scenarios were taken
        relative to the old base, so one commit uses them up: a second one, or one without a dual-updating correct_scenarios on the current
        base before it, raises RuntimeError."""
        sc = self._scenarios
        if sc is None or sc["plan"] is not self._plan:
            raise RuntimeError("commit_scenario() needs a correct_scenarios(update_duals=True) on the current base before it")
        s, pl = self.solver, sc["plan"]
        torch = s.torch
        B, D = sc["step"].shape
        idx = torch.as_tensor(d, dtype=torch.int64, device=sc["step"].device).reshape(-1)
        if idx.numel() == 1:
            idx = idx.expand(B)
        if idx.numel() != B or bool(((idx < 0) | (idx >= D)).any()):
            raise ValueError(f"d must be one scenario index or {B} of them, each in 0 .. {D - 1}")
        rows = torch.arange(B, device=idx.device)
        ok, step = sc["ok"], sc["step"][rows, idx]
        obs = pl["obstacles"]
        if sc["dobs"] is not None:
            okf = ok.reshape((B,) + (1,) * (obs.dim() - 1))
            obs = torch.where(okf, obs + step.reshape(okf.shape) * sc["dobs"][rows, idx], obs)
        self._plan = dict(p=torch.where(ok[:, None], pl["p"] + step[:, None] * sc["dp"][rows, idx], pl["p"]), w=sc["w"][rows, idx],
                          lam_g=sc["lam_g"][rows, idx], lam_x=sc["lam_x"][rows, idx], obstacles=obs, status=pl["status"])
        self._scenarios = None
