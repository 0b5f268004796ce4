"""What the Python sides of LF-Net's two nets (lfnet_desc.py, lfnet_det.py) share: a library handle that destroys itself, the
marshalling of a checkpoint's named arrays into a weights struct, and the from_npz skeleton."""
from __future__ import annotations

import numpy as np

from ._lib import lib

BN_FIELDS = ("gamma", "beta", "moving_mean", "moving_variance")


def resolve_config(default_fn, config):
    """None: the net's defaults; a dict: its fields over the defaults; a config struct: as it is."""
    return default_fn() if config is None else (default_fn(**config) if isinstance(config, dict) else config)


class WeightMarshal:
    """The arrays of `weights` as float32 host pointers for a create call.  `what` names the net in errors and `expected` the
    variables a missing `weights` array is reported against.  The marshal keeps every array it handed out alive."""

    def __init__(self, weights, scope, what, expected):
        self.weights, self.scope, self.what, self.expected, self.keep = weights, scope, what, expected, []

    def arr(self, name, shape):
        """Pointer to `scope/name` as contiguous float32 of `shape`, or None where the array is absent."""
        name = f"{self.scope}/{name}"
        if name not in self.weights:
            return None
        a = np.ascontiguousarray(self.weights[name], np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        self.keep.append(a)
        return a.ctypes.data

    def conv(self, layer, name, wshape):
        """weights (required) and biases of a convolution or fully connected layer."""
        if f"{self.scope}/{name}/weights" not in self.weights:
            raise KeyError(f"{self.what} weights: missing {self.scope}/{name}/weights; expected {self.expected}")
        layer.weights = self.arr(f"{name}/weights", wshape)
        layer.biases = self.arr(f"{name}/biases", (wshape[-1],))

    def bn(self, layer, name, n):
        for k in BN_FIELDS:
            setattr(layer, k, self.arr(f"{name}/{k}", (n,)))


class Handle:
    """An object of the library behind `handle`, destroyed by the symbol named in `_destroy` on close() or collection."""
    _destroy = None
    _h = None

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h is not None and self._h.value:
            getattr(lib(), self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NpzModel(Handle):
    """A model built from a checkpoint's named arrays by the constructor (ws, weights, config, scope).  The net sets, as static
    methods, `_default_config`, `_expected_names` and `_config_from_weights` (its module's functions) and `_counts(cfg, have, scope,
    over)`: the leading arguments of expected_names, from the configuration or else from the stored names."""

    @classmethod
    def _from_npz(cls, ws, path, config, perform_bn, use_bias, scope, over):
        with np.load(path) as z:
            have = {k: z[k] for k in z.files}
        cfg = None if config is None else resolve_config(cls._default_config, config)
        want = cls._expected_names(*cls._counts(cfg, have, scope, over), perform_bn, use_bias, scope)
        missing = [n for n in want if n not in have]
        if missing:
            raise KeyError(f"{path}: missing {missing}; expected the arrays {want}")
        if cfg is None:
            cfg = cls._config_from_weights(have, scope, **over)
        return cls(ws, {n: have[n] for n in want}, cfg, scope)
