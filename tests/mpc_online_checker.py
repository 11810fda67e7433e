"""The checker's restatement of a session (include/mbd_hip.h mbd_plan_mpc_open, DESIGN.md section 1 "N11 session"): the episode
of tests/mpc_checker.py / tests/mpc_delay_checker.py with the state GIVEN at every tick instead of computed — nothing is executed.
oracle.planner.reverse_once for the diffusion steps, mpc_checker's shift and rollout (imported, not edited), numpy for the queue."""
from __future__ import annotations

import numpy as np

from mpc_checker import execute, shift
from mpc_delay_checker import queue_of
from oracle import planner as op


class Session:
    """open: rng = key, Ybar = 0, i_start = Nd - 1, C = rows0 as D blocks of E rows (zeros if None; D = 0: no delay record).
    ``reverse_once``: oracle.planner.reverse_once, or a stand-in with its signature (a noise-shape or ensemble checker's)."""

    def __init__(self, oenv, key, N, H, Nd, temp, K, E, D=0, rows0=None, impl=1, beta0=1e-4, betaT=1e-2, reverse_once=None):
        self.oenv, self.orc = oenv, oenv.orc
        self.N, self.H, self.Nd, self.temp, self.K, self.E, self.D, self.impl = N, H, Nd, temp, K, E, D, impl
        self.sched = self.orc.schedule(beta0, betaT, Nd)
        self.rng = np.asarray(key, np.uint32)
        self.C = queue_of(rows0, D, E, oenv.Nu) if D else None
        self.reverse_once = reverse_once or op.reverse_once
        self.t = 0
        self.reset_mean()

    def reset_mean(self):
        """The next tick is a cold one; the queue stays."""
        self.Ybar, self.i_start, self.cold = np.zeros((self.H, self.oenv.Nu), np.float32), self.Nd - 1, True

    def tick(self, x):
        """dict(mean [H, Nu], rows [E, Nu], head [E, Nu], predicted [S] or None, cold)."""
        E, D, Nu = self.E, self.D, self.oenv.Nu
        keys = self.orc.split(self.rng, 2, self.impl)
        self.rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        frm, shat = x, None
        if D:  # the PLAN's env over the whole queue, in queue order (mpc_delay_checker.episode)
            _, shat = execute(self.oenv, x, self.C.reshape(D * E, Nu))
            frm = shat = np.asarray(shat, np.float32).reshape(-1)
        cold, Ybar = self.cold, self.Ybar
        for i in range(self.i_start, 0, -1):
            r, Ybar, _, _ = self.reverse_once(self.orc, self.oenv, frm, i, r, Ybar, self.sched, self.N, self.H, self.temp, self.impl)
        M = Ybar
        rows = M[:E].copy()  # (copied: -0.0 stays -0.0; unclipped)
        head = rows
        if D:
            head = self.C[0].copy()
            self.C = np.concatenate([self.C[1:], M[:E][None]]).astype(np.float32)
        self.Ybar, self.i_start, self.cold = shift(M, E), self.K, False
        self.t += 1
        return dict(mean=M, rows=rows, head=head, predicted=shat, cold=cold)


def session(oenv, key, states, N, H, Nd, temp, K, E, D=0, rows0=None, reset_at=(), **kw):
    """A session fed ``states`` [T, S], one per tick, with ``reset_mean`` called in front of the ticks of ``reset_at``.  Returns
    dict(means [T, H, Nu], rows [T, E, Nu], heads [T, E, Nu], predicted [T, S] (D > 0, else None))."""
    s = Session(oenv, key, N, H, Nd, temp, K, E, D, rows0, **kw)
    out = []
    for t, x in enumerate(states):
        if t in reset_at:
            s.reset_mean()
        out.append(s.tick(x))
    return dict(means=np.stack([o["mean"] for o in out]), rows=np.stack([o["rows"] for o in out]),
                heads=np.stack([o["head"] for o in out]), predicted=np.stack([o["predicted"] for o in out]) if D else None)
