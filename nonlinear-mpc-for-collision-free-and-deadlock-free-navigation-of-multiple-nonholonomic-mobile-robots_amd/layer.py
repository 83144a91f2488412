"""The NMPC solve as a differentiable torch layer: w* = layer(p, w0, obstacles) with d l / d p and d l / d obstacles for a scalar l(w*).

Forward is one nmpc_solve_batch_duals launch, backward one nmpc_sens_adjoint_batch launch on the solve's own primal-dual point (include/nmpc.h:
the linearisation of the solver's barrier KKT system, O(mu) from the NLP's derivative wherever the NLP has one).  torch carries the tensors and
the tape; all arithmetic happens in libnmpc_hip.so.
"""
from __future__ import annotations

from .solver import NmpcSolver, _torch


def _function():
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class _NmpcSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, layer, p, w0, obstacles):
            s = layer.solver
            r = s.solve_batch(p.detach(), w0.detach(), obstacles=None if obstacles is None else obstacles.detach(), want_duals=True)
            ctx.layer = layer
            ctx.has_obs = obstacles is not None
            ctx.save_for_backward(*([p, r["x"], r["lam_g"], r["lam_x"], r["status"]] + ([obstacles] if ctx.has_obs else [])))
            layer.last = dict(status=r["status"], iters=r["iters"], kkt=r["kkt"], f=r["f"])
            return r["x"]

        @staticmethod
        @once_differentiable
        def backward(ctx, wbar):
            layer = ctx.layer
            saved = ctx.saved_tensors
            p, w, lam_g, lam_x, status = saved[:5]
            obs = saved[5] if ctx.has_obs else None
            want_p, want_o = ctx.needs_input_grad[1], ctx.has_obs and ctx.needs_input_grad[3]
            out = layer.solver.sens_adjoint_batch(p.detach(), w, lam_g, lam_x, wbar, obstacles=None if obs is None else obs.detach(),
                                                  want_pbar=want_p, want_obsbar=want_o)
            ok = (status == 0) & (out["info"] == 0)      # anything else: no derivative to speak of, the row gets zeros
            layer.last["info"] = out["info"]
            layer.last["grad_dropped"] = (~ok).sum()
            gp = go = None
            if want_p:
                gp = torch.where(ok[:, None], out["pbar"], torch.zeros_like(out["pbar"])).reshape(p.shape).to(p.dtype)
            if want_o:
                ob = out["obsbar"]
                go = torch.where(ok.reshape((-1,) + (1,) * (ob.dim() - 1)), ob, torch.zeros_like(ob)).reshape(obs.shape).to(obs.dtype)
            return None, gp, None, go

    return _NmpcSolve


class NmpcLayer:
    """w = layer(p, w0, obstacles=None): the batched solve of `solver` with gradients.

    p [B, n_p] and obstacles ([B, K, 3] or [B, N, K, 3], as in solve_batch) are tensors on the solver's device and may require grad; w0
    [B, n_var] is the initial guess and gets no gradient.  Returns w [B, n_var].  After forward, layer.last holds status, iters, kkt, f of the
    solve; after backward also info (nmpc_sens_adjoint_batch's verdicts) and grad_dropped, the number of rows (a device scalar) whose solve
    status or verdict was not 0 — those rows get zero gradients.  Forward and backward run on the solver's one handle and, as autograd runs
    backward on forward's stream, on one stream."""

    def __init__(self, solver: NmpcSolver):
        if not solver.duals_supported():
            raise RuntimeError("NmpcLayer needs a handle that returns multipliers (the column-per-lane kernel): this one is pinned to kernel 1 or 2")
        self.solver = solver
        self.last = {}
        self._fn = _function()

    def __call__(self, p, w0, obstacles=None):
        return self._fn.apply(self, p, w0, obstacles)
