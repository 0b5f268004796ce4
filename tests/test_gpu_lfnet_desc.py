"""btba_lfnet_descriptors on the MI355X: the stored groups against the fp64 restatement under the stored bars
(tests/golden/lfnet_desc/lfnet_desc_reference.npz, tests/lfnet_desc_ref.py), the tile edges, the release shape under a bar computed
from the restatement's own fp32 error, bit-exactness across calls, batch sizes, slots, frames, counts and chunks, the net inside
LfnetDetector, the C++ host.  One module-scoped workspace.  All figures are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib, lfnet, lfnet_desc

import lfnet_desc_ref as R


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _group(golden, g):
    name, over, _, m = R.GROUPS[g]
    cfg = R.config(**over)
    weights, patches = R.group_model(golden, name)
    return name, cfg, weights, patches, float(golden[f"tol_{name}"])


@pytest.fixture(scope="module")
def model_a(ws, golden):
    """Group a's model with 77 seeded patches and their fp64 results (computed once)."""
    name, cfg, weights, _, tol = _group(golden, 0)
    patches = R.levels(*R.make_patches(77, 77, cfg["patch_size"]))
    d64, r64 = R.forward(weights, cfg, patches, np.float64)
    net = lfnet_desc.LfnetDescriptor(ws, weights, cfg)
    yield dict(cfg=cfg, net=net, patches=patches, d64=d64, r64=r64, tol=tol)
    net.close()


def _errors(desc, d64, r64, cfg):
    """Per patch: lfnet_desc_ref.error (without the norm the device's output IS raw)."""
    return [R.error(desc[i:i + 1], desc[i:i + 1], d64[i:i + 1], r64[i:i + 1], cfg) for i in range(len(desc))]


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stored_groups_against_fp64_under_the_stored_bars(ws, golden, g):
    name, cfg, weights, patches, tol = _group(golden, g)
    d64, r64 = R.forward(weights, cfg, patches, np.float64)
    net = lfnet_desc.LfnetDescriptor(ws, weights, cfg)
    desc = _np(net.describe(_t(patches[None])))[0]
    net.close()
    errs = _errors(desc, d64, r64, cfg)
    ref = _errors(golden[f"{name}/ref_desc"], d64, r64, cfg)
    print(f"group {name}: device vs fp64 {max(errs):.3e}, reference vs fp64 {max(ref):.3e}, tol {tol:.3e}")
    assert np.isfinite(desc).all() and max(errs) <= tol


@pytest.mark.parametrize("m", [1, 31, 32, 33, 77])
def test_tile_edges(model_a, m):
    a = model_a
    desc = _np(a["net"](_t(a["patches"][:m, None])))
    assert desc.shape == (m, a["cfg"]["out_dim"])
    errs = _errors(desc, a["d64"][:m], a["r64"][:m], a["cfg"])
    print(f"m = {m}: device vs fp64 {max(errs):.3e}, tol {a['tol']:.3e}")
    assert max(errs) <= a["tol"]


def test_release_shape_under_the_restatements_own_fp32_error(ws):
    cfg = R.config()
    assert (cfg["channels"], cfg["depth"], cfg["fc_dim"], cfg["out_dim"]) == (64, 3, 512, 256)
    weights = R.model_weights(R.make_model(7, cfg))
    patches = R.levels(*R.make_patches(8, 70, 32))
    d64, r64 = R.forward(weights, cfg, patches, np.float64)
    d32, r32 = R.forward(weights, cfg, patches, np.float32)
    bar = 4.0 * max(_errors(d32, d64, r64, cfg))
    net = lfnet_desc.LfnetDescriptor(ws, weights)              # the default configuration is the release net
    desc = _np(net.describe(_t(patches[None])))[0]
    net.close()
    errs = _errors(desc, d64, r64, cfg)
    print(f"release shape, 70 patches: device vs fp64 {max(errs):.3e}, bar (4 x restatement fp32 vs fp64) {bar:.3e}")
    assert 1e-8 < bar < 1e-5 and np.isfinite(desc).all() and max(errs) <= bar
    assert np.abs(np.linalg.norm(desc.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_one_layer_without_batch_norm_and_bias(ws, golden):
    """Group c's shape with batch norm and biases everywhere except fc1, which has neither (get_model cannot build this, so the bar
    is the restatement's: 4 x its fp32 error against fp64 on the same inputs)."""
    cfg = R.config(**R.GROUPS[2][1])
    weights = R.model_weights(R.make_model(17, cfg))
    for k in ("SimpleDesc/fc1/biases", "SimpleDesc/fc-bn1/gamma", "SimpleDesc/fc-bn1/beta", "SimpleDesc/fc-bn1/moving_mean", "SimpleDesc/fc-bn1/moving_variance"):
        del weights[k]
    del weights["SimpleDesc/bn2/gamma"], weights["SimpleDesc/bn1/beta"]        # NULL gamma = 1, NULL beta = 0
    patches = R.levels(*R.make_patches(18, 9, 32))
    d64, r64 = R.forward(weights, cfg, patches, np.float64)
    bar = 4.0 * max(_errors(R.forward(weights, cfg, patches, np.float32)[0], d64, r64, cfg))
    net = lfnet_desc.LfnetDescriptor(ws, weights, cfg)
    desc = _np(net.describe(_t(patches[None])))[0]
    net.close()
    errs = _errors(desc, d64, r64, cfg)
    print(f"fc1 without batch norm and bias: device vs fp64 {max(errs):.3e}, bar {bar:.3e}")
    assert max(errs) <= bar


def test_same_patch_same_bits_whatever_the_batch(model_a):
    import torch
    a = model_a
    net, P, D = a["net"], a["cfg"]["patch_size"], a["cfg"]["out_dim"]
    all77 = _t(a["patches"][None])
    first = _np(net.describe(all77))
    assert np.array_equal(_bits(first), _bits(_np(net.describe(all77))))                      # two calls
    alone = _np(net.describe(_t(a["patches"][40][None, None])))[0, 0]
    assert np.array_equal(_bits(alone), _bits(first[0, 40]))                                   # alone and at slot 40 of 77
    three = np.zeros((3, 5, P, P), np.float32)
    three[:] = a["patches"][:15].reshape(3, 5, P, P)
    three[2, 3] = a["patches"][40]
    got = _np(net.describe(_t(three)))
    assert np.array_equal(_bits(got[2, 3]), _bits(alone))                                      # in frame 2 of 3
    assert np.array_equal(_bits(got[0]), _bits(first[0, :5]))
    # counts: frames of 77 slots with 0, 5 and all of them
    slots = 77
    batch = _t(np.stack([a["patches"]] * 3))
    full = _np(net.describe(batch))
    for counts in ([0, 5, slots], [slots, 0, 64], [1, 33, 0]):
        masked = _np(net.describe(batch, torch.tensor(counts, dtype=torch.int32, device="cuda")))
        for f, c in enumerate(counts):
            assert np.array_equal(_bits(masked[f, :c]), _bits(full[f, :c])), (counts, f)
            assert not masked[f, c:].any() and not np.signbit(masked[f, c:]).any(), (counts, f)
    for f in range(3):
        assert np.array_equal(_bits(full[f]), _bits(first[0]))


def test_more_patches_than_one_pass_holds(model_a):
    """3 x 700 slots = 2100 patches: two passes over the layers (2048 patches each); the bits of a patch do not depend on the pass."""
    a = model_a
    idx = np.arange(2100) % 77
    batch = a["patches"][idx].reshape(3, 700, *a["patches"].shape[1:])
    got = _np(a["net"].describe(_t(batch))).reshape(2100, -1)
    want = _np(a["net"](_t(a["patches"][:, None])))
    assert np.array_equal(_bits(got), _bits(want[idx]))


def test_empty_calls_and_a_model_of_another_workspace(ws, model_a):
    import torch
    from bundletrack_amd.optimizer import Workspace
    a = model_a
    P, D = a["cfg"]["patch_size"], a["cfg"]["out_dim"]
    assert tuple(a["net"].describe(torch.empty((0, 5, P, P), dtype=torch.float32, device="cuda")).shape) == (0, 5, D)
    assert tuple(a["net"].describe(torch.empty((2, 0, P, P), dtype=torch.float32, device="cuda")).shape) == (2, 0, D)
    other = Workspace()
    p, d = _t(a["patches"][None]), torch.empty((1, 77, D), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    assert L.btba_lfnet_descriptors(other.handle, a["net"].handle, 1, 77, p.data_ptr(), None, d.data_ptr()) == _lib.BTBA_EINVAL
    assert L.btba_lfnet_descriptors(ws.handle, a["net"].handle, 1, 77, p.data_ptr(), None, d.data_ptr()) == _lib.BTBA_OK
    torch.cuda.synchronize()
    other.close()
    with pytest.raises(ValueError):
        a["net"].describe(_t(np.zeros((1, 3, P + 1, P), np.float32)))


class _ScoreNet:
    """A fixed-weight conv 'score net': S score maps at int(H / s + 0.5) and a unit orientation map."""

    def __init__(self, scale_factors):
        import torch
        g = torch.Generator().manual_seed(11)
        self.sf = scale_factors
        self.w = torch.randn((3, 1, 5, 5), generator=g).cuda()

    def __call__(self, gray):
        import torch
        F = torch.nn.functional
        H, W = gray.shape[-2:]
        maps = []
        for s in self.sf:
            x = F.interpolate(gray, size=(int(H / s + 0.5), int(W / s + 0.5)), mode="bilinear", align_corners=False)
            maps.append(F.conv2d(x, self.w[:1], padding=2)[:, 0])
        o = F.conv2d(gray, self.w[1:], padding=2)
        o = o / o.norm(dim=1, keepdim=True).clamp_min(1e-6)
        return maps, o.permute(0, 2, 3, 1).contiguous()


def test_inside_the_detector(ws, golden):
    import torch
    name, cfg, weights, _, _ = _group(golden, 2)                                                # P = 32, the keypoint head's patch size
    net = lfnet_desc.LfnetDescriptor(ws, weights, cfg)
    sf = (2.0 ** 0.5, 1.0, 2.0 ** -0.5)
    det = lfnet.LfnetDetector(ws, _ScoreNet(sf), net, sf, dict(top_k=64))
    gray = torch.rand((1, 1, 96, 112), generator=torch.Generator().manual_seed(5)).cuda()
    kpts, desc = det(None, gray)
    m = int(det.last["n_kpts_host"][0])
    assert 0 < m <= 64 and tuple(kpts.shape) == (m, 2) and tuple(desc.shape) == (m, cfg["out_dim"])
    again = _np(net.describe(det.last["patches"], det.last["n_kpts"]))[0]
    assert np.array_equal(_bits(_np(desc)), _bits(again[:m])) and not again[m:].any()
    assert np.abs(np.linalg.norm(_np(desc).astype(np.float64), axis=1) - 1.0).max() < 1e-6
    net.close()


def _host_struct(weights, cfg):
    W = _lib.LfnetDescWeights()
    keep = []
    for i, (layer, bn) in enumerate(R.layer_scopes(cfg["depth"])):
        dst = W.conv[i] if i < cfg["depth"] else (W.fc1 if layer == "fc1" else W.fc2)
        for field, name in [("weights", f"SimpleDesc/{layer}/weights"), ("biases", f"SimpleDesc/{layer}/biases")] + \
                           ([(k, f"SimpleDesc/{bn}/{k}") for k in ("gamma", "beta", "moving_mean", "moving_variance")] if bn else []):
            if name in weights:
                keep.append(np.ascontiguousarray(weights[name], np.float32))
                setattr(dst, field, keep[-1].ctypes.data)
    return W, keep


@pytest.mark.parametrize("via_desc_net", [0, 1])
def test_cpp_host_equals_python(ws, golden, via_desc_net):
    import torch
    _lib.build_host_cpp()                                                                       # a no-op after build()
    drv = C.CDLL(_lib.LFNET_DESC_DRIVER)
    drv.lfnet_desc_driver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    name, cfg, weights, patches, _ = _group(golden, 1)
    net = lfnet_desc.LfnetDescriptor(ws, weights, cfg)
    batch = _t(np.stack([patches, patches[::-1]]))                                              # 2 frames x 5 slots
    counts = None if via_desc_net else torch.tensor([3, 5], dtype=torch.int32, device="cuda")
    want = _np(net.describe(batch, counts))
    net.close()
    W, keep = _host_struct(weights, cfg)
    c = _lib.lfnet_desc_config(**cfg)
    out = torch.full((2, 5, cfg["out_dim"]), 7.0, dtype=torch.float32, device="cuda")
    rc = drv.lfnet_desc_driver(ws.handle, C.addressof(c), C.addressof(W), 2, 5, batch.data_ptr(), None if counts is None else counts.data_ptr(),
                               out.data_ptr(), via_desc_net)
    assert rc == 0
    got = _np(out)
    if via_desc_net:
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and (got[1] == 7.0).all()         # the DescFn describes one frame
    else:
        assert np.array_equal(_bits(got), _bits(want)) and not got[0, 3:].any()
    c.out_dim = 24
    assert drv.lfnet_desc_driver(ws.handle, C.addressof(c), C.addressof(W), 2, 5, batch.data_ptr(), None, out.data_ptr(), 0) == _lib.BTBA_EINVAL
