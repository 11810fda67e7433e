"""Terminal value nets (include/mbd_hip.h mbd_value; DESIGN.md section 1 "N16 value"): the record's fields as a dataclass, the
import of a torch net, the ``.npz`` format ``mpc.py --value`` reads and ``mbd_hip.scripts.fit_value`` writes."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .. import _capi

ACTS = {"relu": _capi.VALUE_RELU, "tanh": _capi.VALUE_TANH}


def terminal_scale(weight: float, Hsample: int) -> float:
    """The record's ``scale`` that weighs V like ``weight`` further reward rows: a plan's reward is the MEAN of its Hsample rows,
    so one more row's worth of reward is 1 / Hsample."""
    return float(weight) / float(Hsample)


@dataclass
class ValueNet:
    """The fields of ``mbd_value``.  ``W[l]`` is layer l + 1's weight [width, inputs] — ``torch.nn.Linear.weight``'s layout —,
    ``b[l]`` its bias; the last layer has one output and no activation."""
    W: List[np.ndarray]
    b: List[np.ndarray]
    act: str = "relu"
    center: Optional[np.ndarray] = None
    in_scale: Optional[np.ndarray] = None
    rel_xy: bool = False
    scale: float = 1.0

    def __post_init__(self):
        if self.act not in ACTS:
            raise ValueError(f"act={self.act!r}: one of {sorted(ACTS)}")
        if len(self.W) != len(self.b) or not self.W:
            raise ValueError(f"a value net has as many weights as biases and at least one layer, not {len(self.W)} and {len(self.b)}")
        self.W = [np.ascontiguousarray(w, np.float32) for w in self.W]
        self.b = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in self.b]
        for l, w in enumerate(self.W):
            if w.ndim != 2 or w.shape[0] != self.b[l].size or (l and w.shape[1] != self.W[l - 1].shape[0]):
                raise ValueError(f"layer {l + 1}: weight {w.shape} does not fit its bias [{self.b[l].size}] and the layer before")
        for name in ("center", "in_scale"):
            x = getattr(self, name)
            if x is not None:
                setattr(self, name, np.ascontiguousarray(x, np.float32).reshape(-1))

    @property
    def n_in(self) -> int:
        return int(self.W[0].shape[1])

    @property
    def widths(self) -> List[int]:
        return [int(w.shape[0]) for w in self.W]

    def record(self, scale: float = None) -> "_capi.Value":
        """The ``mbd_value`` of this net (its pointers read this object's arrays: keep it alive until the set call has returned).
        Nets the record cannot hold go to the library, which names the field — except a layer count beyond its arrays."""
        if len(self.W) > _capi.VALUE_MAX_LAYERS:
            raise ValueError(f"a value record holds 1..{_capi.VALUE_MAX_LAYERS} layers, not {len(self.W)}")
        fp = C.POINTER(C.c_float)
        rec = _capi.Value()
        for l, (w, b) in enumerate(zip(self.W, self.b)):
            rec.W[l], rec.b[l] = w.ctypes.data_as(fp), b.ctypes.data_as(fp)
            rec.width[l] = w.shape[0]
        if self.center is not None:
            rec.center = self.center.ctypes.data_as(fp)
        if self.in_scale is not None:
            rec.in_scale = self.in_scale.ctypes.data_as(fp)
        rec.n_in, rec.n_layers = self.n_in, len(self.W)
        rec.act = ACTS[self.act]
        rec.flags = _capi.VALUE_REL_XY if self.rel_xy else 0
        rec.scale = float(self.scale if scale is None else scale)
        return rec

    @classmethod
    def from_torch(cls, net, center=None, in_scale=None, rel_xy: bool = False, scale: float = 1.0) -> "ValueNet":
        """From a ``torch.nn.Sequential`` of ``Linear`` layers with ONE kind of activation (``ReLU`` or ``Tanh``) between them and
        none behind the last."""
        import torch.nn as nn
        W, b, acts = [], [], []
        mods = list(net)
        for m in mods:
            if isinstance(m, nn.Linear):
                if len(acts) != len(W):
                    raise ValueError("two Linear layers follow each other without an activation")
                W.append(m.weight.detach().cpu().numpy())
                b.append(m.bias.detach().cpu().numpy() if m.bias is not None else np.zeros(m.out_features, np.float32))
            elif isinstance(m, (nn.ReLU, nn.Tanh)):
                if len(acts) != len(W) - 1:
                    raise ValueError("an activation must follow a Linear layer")
                acts.append("relu" if isinstance(m, nn.ReLU) else "tanh")
            else:
                raise ValueError(f"{type(m).__name__}: a value net is Linear / ReLU / Tanh layers")
        if not W or len(acts) != len(W) - 1:
            raise ValueError("the net must end in a Linear layer")
        if len(set(acts)) > 1:
            raise ValueError("one activation for all hidden layers: the net mixes ReLU and Tanh")
        return cls(W, b, acts[0] if acts else "relu", center, in_scale, rel_xy, scale)

    def save(self, path) -> None:
        arrs = {f"W{l}": w for l, w in enumerate(self.W)}
        arrs.update({f"b{l}": x for l, x in enumerate(self.b)})
        if self.center is not None:
            arrs["center"] = self.center
        if self.in_scale is not None:
            arrs["in_scale"] = self.in_scale
        np.savez(path, n_layers=np.int32(len(self.W)), act=np.str_(self.act), rel_xy=np.int32(self.rel_xy),
                 scale=np.float32(self.scale), **arrs)

    @classmethod
    def load(cls, path) -> "ValueNet":
        with np.load(path) as z:
            n = int(z["n_layers"])
            return cls([z[f"W{l}"] for l in range(n)], [z[f"b{l}"] for l in range(n)], str(z["act"]),
                       z["center"] if "center" in z else None, z["in_scale"] if "in_scale" in z else None,
                       bool(int(z["rel_xy"])), float(z["scale"]))
