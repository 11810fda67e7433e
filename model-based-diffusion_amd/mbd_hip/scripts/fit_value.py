"""Fit a terminal value net (include/mbd_hip.h mbd_value) to logged episodes — a Monte-Carlo fit, the smallest thing that gives
``mpc.py --value`` a net without another code base.

    python -m mbd_hip.scripts.fit_value --episodes results/hopper/mpc_episode.npz ... --hidden 64 64 --discount 0.99 \
        --steps_ahead 50 --out value.npz

Input: the ``states`` [T + 1, S] (or [P, T + 1, S]) and ``rewards`` [T * E] (or [P, T * E]) ``mpc.py`` saves.  The state of tick t
is the state in front of control step t * E.  Target of tick t: the discounted sum of the next ``steps_ahead`` rewards,
sum_j discount ** j * r[t E + j]; ticks with fewer rewards left are dropped (a truncated sum is not the same quantity).  ``center``
and ``in_scale`` are the inputs' means and inverse standard deviations (under ``--rel_xy`` of the states as the record sees them;
an input that never moves is masked).  Training is plain torch on the CPU: Adam on the mean squared error of the standardised target,
the last layer rescaled afterwards so that V is in reward units."""
import argparse
import json

import numpy as np

from ..planners.value import ValueNet

LINK = 13


def load_episodes(paths):
    """(states [n, T + 1, S], rewards [n, T E]) lists of the episodes in the files (a batch file holds several)."""
    eps = []
    for p in paths:
        with np.load(p) as z:
            s, r = np.asarray(z["states"], np.float32), np.asarray(z["rewards"], np.float32)
        if s.ndim == 2:
            s, r = s[None], r[None]
        eps += [(s[k].reshape(s.shape[1], -1), r[k].reshape(-1)) for k in range(s.shape[0])]
    return eps


def targets(eps, discount: float, steps_ahead: int):
    """(X [n, S], y [n]): every tick's state with ``steps_ahead`` rewards ahead of it, and their discounted sum (float64 sums)."""
    X, y = [], []
    g = float(discount) ** np.arange(steps_ahead)
    for s, r in eps:
        T = s.shape[0] - 1
        if T < 1 or r.size % T:
            raise ValueError(f"an episode of {T} ticks with {r.size} rewards: rewards must be [T * E]")
        E = r.size // T
        for t in range(T):
            if t * E + steps_ahead <= r.size:
                X.append(s[t])
                y.append(float(np.dot(g, r[t * E:t * E + steps_ahead].astype(np.float64))))
    if not X:
        raise ValueError(f"no tick has {steps_ahead} rewards ahead of it: shorten --steps_ahead or log longer episodes")
    return np.stack(X).astype(np.float32), np.asarray(y, np.float32)


def _seen(X, rel_xy: bool):
    X = np.array(X, np.float32)
    if rel_xy:
        x0, y0 = X[:, 0].copy(), X[:, 1].copy()
        X[:, 0::LINK] -= x0[:, None]
        X[:, 1::LINK] -= y0[:, None]
    return X


def fit(X, y, hidden=(64, 64), act="relu", rel_xy=False, steps=2000, lr=3e-3, seed=0, log=None) -> "tuple[ValueNet, dict]":
    """The fitted net and dict(loss, loss_const): the final mean squared error and the constant predictor's, in target units."""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    Xs = _seen(X, rel_xy)
    center = Xs.mean(axis=0).astype(np.float32)
    sd = Xs.std(axis=0)
    in_scale = np.where(sd > 1e-6, 1.0 / np.maximum(sd, 1e-6), 0.0).astype(np.float32)
    xin = torch.tensor((Xs - center) * in_scale)
    y_mean, y_sd = float(y.mean()), float(max(y.std(), 1e-6))
    yt = torch.tensor((y - y_mean) / y_sd).reshape(-1, 1)
    layers, k = [], Xs.shape[1]
    for w in hidden:
        layers += [nn.Linear(k, int(w)), nn.ReLU() if act == "relu" else nn.Tanh()]
        k = int(w)
    layers.append(nn.Linear(k, 1))
    net = nn.Sequential(*layers)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    for it in range(int(steps)):
        opt.zero_grad()
        loss = ((net(xin) - yt) ** 2).mean()
        loss.backward()
        opt.step()
        if log and (it % max(1, int(steps) // 10) == 0):
            log(f"step {it}: loss {float(loss.detach()) * y_sd ** 2:.6g}")
    with torch.no_grad():  # V in reward units: the last layer carries the target's scale and mean
        net[-1].weight.mul_(y_sd)
        net[-1].bias.mul_(y_sd).add_(y_mean)
        final = float(((net(xin).reshape(-1) - torch.tensor(y)) ** 2).mean())
    vn = ValueNet.from_torch(net, center=center, in_scale=in_scale, rel_xy=rel_xy, scale=1.0)
    return vn, dict(loss=final, loss_const=float(y.var()), samples=int(len(y)))


def main(argv=None) -> dict:
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--episodes", nargs="+", required=True, help="mpc_episode.npz files")
    p.add_argument("--hidden", nargs="*", type=int, default=[64, 64], help="hidden widths (none: a linear value)")
    p.add_argument("--act", default="relu", choices=["relu", "tanh"])
    p.add_argument("--discount", type=float, default=0.99)
    p.add_argument("--steps_ahead", type=int, default=50)
    p.add_argument("--rel_xy", action="store_true", help="rigid-body envs: x and y relative to link 0 (MBD_VALUE_REL_XY)")
    p.add_argument("--steps", type=int, default=2000, help="Adam steps (full batch)")
    p.add_argument("--lr", type=float, default=3e-3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", required=True)
    a = p.parse_args(argv)
    import sys
    X, y = targets(load_episodes(a.episodes), a.discount, a.steps_ahead)
    vn, info = fit(X, y, a.hidden, a.act, a.rel_xy, a.steps, a.lr, a.seed, log=lambda m: print(m, file=sys.stderr))
    vn.save(a.out)
    res = dict(out=a.out, n_in=vn.n_in, widths=vn.widths, act=vn.act, rel_xy=vn.rel_xy, discount=a.discount,
               steps_ahead=a.steps_ahead, **info)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
