"""Writes tests/golden/vos_net/vos_net_reference.npz: seeds, inputs and the reference's own results for them.

    python tests/golden/make_vos_net_golden.py          (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/vos_ref.py)

The reference's transductive-vos.pytorch/modeling/backbone/resnet.py and modeling/network.py are loaded by path, its own VOSNet is
built, given the seeded arrays of vos_net_ref.make_model and run in eval mode on CPU torch, in fp32 and in fp64.  VOSNet.__init__
hard-codes pretrained=True, which calls model_zoo.load_url: before anything is constructed the loaded resnet module's `model_zoo` is
replaced by an object whose load_url returns {} (asserted), so nothing here can reach the network.  A group whose depths are not
those of a stock constructor gets its ResNet from the reference's own ResNet class with the group's depths.  The models are
regenerated from their seeds, never stored.  Per group of vos_net_ref.GROUPS:
  <g>/model_seed, <g>/photo_seed   the seeds
  <g>/photos, <g>/photos@mult      the frames as int8 levels and one fp32 multiplier
  <g>/ref                          the reference's fp32 output [n, 256, Hd, Wd]
  <g>/keys                         the sorted names of VOSNet.state_dict()
  <g>/crc_model, <g>/crc_photos    CRC-32 of the regenerated levels (vos_net_ref.crc): generator drift is a clear failure
  <g>/err_ref32, <g>/err_chain32   max |y - y64| / max |y64| per frame of the reference's fp32 run and of the restatement's fp32
                                   k-ordered chain, both against the reference's fp64 run
  tol_<g>                          4 x max(err_ref32, err_chain32)
The file is written only if every bar lies in (1e-7, 1e-4) and the restatement in fp64 agrees with the reference in fp64 to 1e-10."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vos_net_ref as R  # noqa: E402
from vos_ref import reference_dir  # noqa: E402

STOCK = {(R.BASIC, (2, 2, 2, 2)): "resnet18", (R.BOTTLENECK, (3, 4, 6, 3)): "resnet50", (R.BOTTLENECK, (3, 4, 23, 3)): "resnet101"}


class _NoDownload:
    """Stands in for torch.utils.model_zoo inside the reference's resnet module."""
    calls = 0

    def load_url(self, *a, **k):
        _NoDownload.calls += 1
        return {}


def reference_modules():
    """(resnet, network) of the reference loaded by path under the package names network.py imports them by."""
    root = os.path.join(reference_dir(), "transductive-vos.pytorch", "modeling")
    if not os.path.exists(os.path.join(root, "network.py")):
        raise SystemExit(f"no reference checkout at {reference_dir()}")
    for name in ("modeling", "modeling.backbone", "modeling.sync_batchnorm"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sync = types.ModuleType("modeling.sync_batchnorm.batchnorm")          # network.py needs only the name; sync_bn stays False
    sync.SynchronizedBatchNorm2d = None
    sys.modules[sync.__name__] = sync

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    resnet = load("modeling.backbone.resnet", os.path.join(root, "backbone", "resnet.py"))
    resnet.model_zoo = _NoDownload()
    network = load("modeling.network", os.path.join(root, "network.py"))
    return resnet, network


def build(resnet, network, cfg):
    """The reference's VOSNet with the depths of `cfg`."""
    assert isinstance(resnet.model_zoo, _NoDownload)
    key = (cfg["block"], tuple(cfg["layers"]))
    kind = "resnet18" if cfg["block"] == R.BASIC else "resnet50"
    if key in STOCK:
        return network.VOSNet(model=STOCK[key])
    block = resnet.BasicBlock if cfg["block"] == R.BASIC else resnet.Bottleneck
    stock = getattr(network, kind)
    setattr(network, kind, lambda pretrained=False, BatchNorm=None: resnet.ResNet(block, list(cfg["layers"]), BatchNorm=BatchNorm))
    try:
        return network.VOSNet(model=kind)
    finally:
        setattr(network, kind, stock)


def main():
    import torch
    torch.manual_seed(0)
    resnet, network = reference_modules()
    out = {}
    for g, (name, over, (n, H, W)) in enumerate(R.GROUPS):
        cfg = R.config(**over)
        q = R.make_model(R.MODEL_SEED + g, cfg)
        weights = R.model_weights(q)
        lev, mult = R.make_photos(R.PHOTO_SEED + g, n, H, W)
        photos = R.levels(lev, mult)
        net = build(resnet, network, cfg)
        sd = net.state_dict()
        keys = sorted(sd)
        assert sorted(k for k in keys if not k.endswith("num_batches_tracked")) == sorted(weights), name
        net.load_state_dict({k: (torch.from_numpy(weights[k]) if k in weights else v) for k, v in sd.items()}, strict=True)
        net.eval()
        with torch.no_grad():
            ref32 = net(torch.from_numpy(photos)).numpy()
            ref64 = net.double()(torch.from_numpy(photos.astype(np.float64))).numpy()
        assert ref32.dtype == np.float32 and ref64.dtype == np.float64
        assert ref32.shape == (n, R.OUT_C, R.out_size(H), R.out_size(W)) == (n, 256, -(-H // 8), -(-W // 8))
        y64 = R.forward(weights, cfg, photos, np.float64)
        agree = R.error(y64, ref64)
        err_ref, err_chain = R.error(ref32, ref64), R.error(R.forward(weights, cfg, photos, np.float32), ref64)
        tol = 4.0 * max(err_ref, err_chain)
        print(f"group {name}: restatement fp64 vs reference fp64 {agree:.3e}; reference fp32 {err_ref:.3e}, fp32 chain {err_chain:.3e}, bar {tol:.3e}; "
              f"max |y64| {np.abs(ref64).max():.3e}")
        assert agree < 1e-10, (name, agree)
        assert 1e-7 < tol < 1e-4, (name, tol)
        out[f"{name}/model_seed"], out[f"{name}/photo_seed"] = np.int64(R.MODEL_SEED + g), np.int64(R.PHOTO_SEED + g)
        out[f"{name}/photos"], out[f"{name}/photos@mult"] = lev, mult
        out[f"{name}/ref"] = ref32
        out[f"{name}/keys"] = np.array(keys)
        out[f"{name}/crc_model"], out[f"{name}/crc_photos"] = np.uint32(R.crc(q)), np.uint32(R.crc((lev, mult)))
        out[f"{name}/err_ref32"], out[f"{name}/err_chain32"] = np.float64(err_ref), np.float64(err_chain)
        out[f"tol_{name}"] = np.float64(tol)
    assert _NoDownload.calls >= 1                                         # the stock resnet50 went through the replaced load_url
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
    assert os.path.getsize(R.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
