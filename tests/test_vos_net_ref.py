"""The segmentation backbone without a GPU: the numpy restatement (tests/vos_net_ref.py) against the reference's own stored results
(tests/golden/vos_net/vos_net_reference.npz, written by tests/golden/make_vos_net_golden.py from the reference's VOSNet on CPU torch),
the output-size rule, the checkpoint's names, the generators' CRCs, and the host-side plan and weight re-layout
(bundletrack_amd/csrc/btba_vos_net_plan.hpp) in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bundletrack_amd import _lib, vos_net

import vos_net_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def groups(golden):
    return [R.group(golden, g) for g in range(len(R.GROUPS))]


@pytest.mark.parametrize("g", [0, 1, 2])
def test_restatement_against_the_references_stored_output(groups, golden, g):
    G = groups[g]
    n, H, W = R.GROUPS[g][2]
    y64 = R.forward(G["weights"], G["cfg"], G["photos"], np.float64)
    assert y64.shape == G["ref"].shape == (n, 256, -(-H // 8), -(-W // 8)) and G["ref"].dtype == np.float32
    err = R.error(G["ref"], y64)
    print(f"group {G['name']}: reference fp32 vs restatement fp64 {err:.3e}, stored {float(golden[G['name'] + '/err_ref32']):.3e}, bar {G['tol']:.3e}")
    assert 1e-7 < G["tol"] < 1e-4
    assert err <= G["tol"]
    # the bar is 4 x the larger of the two stored errors
    assert G["tol"] == 4.0 * max(float(golden[f"{G['name']}/err_ref32"]), float(golden[f"{G['name']}/err_chain32"]))


@pytest.mark.parametrize("g", [0, 1, 2])
def test_fp32_chain_stays_within_a_quarter_of_the_bar(groups, g):
    """The k-ordered fp32 chain is one of the two errors the bar is four times the larger of.  The fp64 side here is the restatement's,
    the maker's was the reference's; the maker lets the two differ by 1e-10, which is the slack."""
    G = groups[g]
    y64 = R.forward(G["weights"], G["cfg"], G["photos"], np.float64)
    y32 = R.forward(G["weights"], G["cfg"], G["photos"], np.float32)
    assert y32.dtype == np.float32
    err = R.error(y32, y64)
    print(f"group {G['name']}: fp32 chain vs fp64 {err:.3e}, a quarter of the bar {G['tol'] / 4:.3e}")
    assert 0.0 < err <= G["tol"] / 4 + 1e-10


def test_out_size_is_ceil_of_an_eighth():
    L = _lib.lib()
    hd, wd = C.c_int32(), C.c_int32()
    for H in range(1, 201):
        assert R.out_size(H) == -(-H // 8)
        assert L.btba_vos_net_out_size(H, 201 - H, C.byref(hd), C.byref(wd)) == _lib.BTBA_OK
        assert (hd.value, wd.value) == (-(-H // 8), -(-(201 - H) // 8)) == vos_net.out_size(H, 201 - H)
    for H, W in ((0, 8), (8, 0), (-1, 8), (4097, 8), (8, 4097)):
        assert L.btba_vos_net_out_size(H, W, C.byref(hd), C.byref(wd)) == _lib.BTBA_EINVAL
    assert L.btba_vos_net_out_size(8, 8, None, C.byref(wd)) == _lib.BTBA_EINVAL
    assert L.btba_vos_net_out_size(4096, 4096, C.byref(hd), C.byref(wd)) == _lib.BTBA_OK and (hd.value, wd.value) == (512, 512)


@pytest.mark.parametrize("g", [0, 1, 2])
def test_expected_names_are_the_state_dicts(groups, g):
    G = groups[g]
    stored = [k for k in G["keys"] if not k.endswith("num_batches_tracked")]
    assert len(stored) < len(G["keys"])                     # the reference's batch norms do carry num_batches_tracked
    names = vos_net.expected_names(G["cfg"])
    assert sorted(names) == stored == sorted(G["weights"])
    assert len(names) == 5 * len(R.layer_table(G["cfg"])) == 5 * _lib.lib().btba_vos_net_layer_count(C.byref(_lib.vos_net_config(**G["cfg"])))
    cfg = vos_net.config_from_state_dict({("module." + k): None for k in G["keys"]})
    assert (int(cfg.block), list(cfg.layers)) == (G["cfg"]["block"], G["cfg"]["layers"])


def test_default_configuration_and_layer_counts():
    c = _lib.vos_net_config()
    assert (int(c.block), list(c.layers), float(c.bn_eps)) == (1, [3, 4, 6, 3], float(np.float32(1e-5)))
    count = lambda **kw: _lib.lib().btba_vos_net_layer_count(C.byref(_lib.vos_net_config(**kw)))
    assert count() == 1 + 3 * 16 + 3 + 1 == 53              # resnet50: stem, 16 bottlenecks, three downsamples, adjust_dim
    assert count(block=0, layers=[2, 2, 2, 2]) == 1 + 2 * 8 + 2 == 19
    assert count(layers=[3, 4, 23, 3]) == 1 + 3 * 33 + 3 + 1 == 104
    for bad in (dict(block=2), dict(block=-1), dict(layers=[0, 1, 1, 1]), dict(layers=[1, 1, 1, 65]), dict(bn_eps=-1.0), dict(bn_eps=float("nan"))):
        assert count(**bad) == -1, bad
    assert _lib.lib().btba_vos_net_layer_count(None) == -1


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stored_crcs_match_the_regenerated_levels(groups, golden, g):
    G = groups[g]
    name = G["name"]
    assert int(golden[f"{name}/model_seed"]) == R.MODEL_SEED + g and int(golden[f"{name}/photo_seed"]) == R.PHOTO_SEED + g
    assert R.crc(G["q"]) == int(golden[f"{name}/crc_model"]), "vos_net_ref.make_model no longer draws what the golden file was made from"
    n, H, W = R.GROUPS[g][2]
    lev, mult = R.make_photos(int(golden[f"{name}/photo_seed"]), n, H, W)
    assert R.crc((lev, mult)) == int(golden[f"{name}/crc_photos"])
    assert np.array_equal(lev, golden[f"{name}/photos"]) and mult == golden[f"{name}/photos@mult"]


def _hex(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, np.float32).ravel().view(np.uint32))


def test_plan_and_relayout_under_sanitizers(tmp_path):
    """btba_vos_net_plan.hpp alone, in tests/cpp/vos_net_host.cpp built with AddressSanitizer and UBSan: the plan's convolutions are
    vos_net_ref.layer_table's with consistent image sizes, buffers and arena offsets, the re-laid weight is the [K][N] transpose in
    (ky, kx, c_in) order, the folded (scale, shift) are float32 of vos_net_ref.fold, the verdicts are the rules of include/btba.h, and
    the sanitizers report nothing."""
    exe = str(tmp_path / "vos_net_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vos_net_host.cpp"), "-o", exe])
    eps = np.float32(1e-5)
    plans = [(R.config(**over), H, W) for _, over, (_, H, W) in R.GROUPS]
    plans += [(R.config(block=0, layers=[2, 2, 2, 2]), 65, 63), (R.config(layers=[3, 4, 23, 3]), 480, 640), (R.config(), 1, 1), (R.config(), 480, 640)]
    bad = [dict(block=2), dict(layers=[0, 1, 1, 1]), dict(layers=[1, 65, 1, 1])]
    lines = [f"P {c['block']} {' '.join(map(str, c['layers']))} {_hex(eps)} {H} {W}" for c, H, W in plans]
    lines += [f"P {c['block']} {' '.join(map(str, c['layers']))} {_hex(eps)} 8 8" for c in (R.config(**b) for b in bad)]
    # records: (cout, cin, k), all present or one array missing / with a NaN / a variance that cancels eps
    rs = np.random.default_rng(3)
    records = []
    for cout, cin, k in ((64, 3, 7), (8, 16, 3), (16, 8, 1)):
        full = dict(weight=rs.standard_normal((cout, cin, k, k)), bn_weight=rs.uniform(0.5, 1.5, cout), bn_bias=rs.standard_normal(cout),
                    running_mean=rs.standard_normal(cout), running_var=rs.uniform(0.5, 1.5, cout))
        full = {n: v.astype(np.float32) for n, v in full.items()}
        records.append((cout, cin, k, full, True))
        for name in full:
            records.append((cout, cin, k, {n: v for n, v in full.items() if n != name}, False))
            a = {n: v.copy() for n, v in full.items()}
            a[name].ravel()[-1] = np.nan
            records.append((cout, cin, k, a, False))
        a = {n: v.copy() for n, v in full.items()}
        a["running_var"][-1] = -eps
        records.append((cout, cin, k, a, False))
    order = ("weight", "bn_weight", "bn_bias", "running_mean", "running_var")
    for cout, cin, k, a, _ in records:
        lines.append(f"L {cout} {cin} {k} {_hex(eps)} " + " ".join(str(int(n in a)) for n in order) + " " + " ".join(_hex(a[n]) for n in order if n in a))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = iter(run.stdout.splitlines())
    for cfg, H, W in plans:
        table = R.layer_table(cfg)
        head = next(out).split()
        ok, n_layers, arena, buffer_floats, Hd, Wd = (int(v) for v in head[:6])
        assert ok == 1 and n_layers == len(table) and (Hd, Wd) == (-(-H // 8), -(-W // 8))
        convs = [[int(v) for v in next(out).split()] for _ in range(n_layers)]
        assert sorted(c[0] for c in convs) == list(range(n_layers)) and convs[0][0] == 0
        sizes, regions, biggest, macs = {}, [], 0, 0.0
        for i, (layer, ks, stride, pad, cin, cout, src, dst, res, relu, Hi, Wi, Ho, Wo, w, scale, shift) in enumerate(convs):
            name, _, t_cout, t_cin, t_k, t_stride = table[layer]
            assert (ks, stride, pad, cin, cout) == (t_k, t_stride, t_k // 2, t_cin, t_cout), name
            assert (Ho, Wo) == ((Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1)
            if i == 0:
                assert (Hi, Wi, src, dst, res, relu) == (H, W, -1, 1, -1, 1)
                sizes[0] = ((Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1)          # the pool takes A to X
            else:
                assert sizes[src] == (Hi, Wi) and src != dst and 0 <= src < 4 and 0 <= dst <= 4 and res != src
                if res >= 0:                                                # the shortcut has the output's size; it may be the output itself
                    assert sizes[res] == (Ho, Wo) and name.endswith("conv3" if cfg["block"] else "conv2")
                assert relu == (0 if name.endswith("downsample.0") or name == "adjust_dim" else 1)
            sizes[dst] = (Ho, Wo)
            if dst != 4:
                biggest = max(biggest, Ho * Wo * cout)
            macs += float(Ho * Wo * cout) * ks * ks * cin
            regions += [(w, ks * ks * cin * cout), (scale, cout), (shift, cout)]
        assert convs[-1][7] == 4 and all(c[7] != 4 for c in convs[:-1]) and sizes[4] == (Hd, Wd) and convs[-1][5] == 256
        assert buffer_floats == biggest and float(head[6]) == macs
        regions.sort()
        assert all(at % 64 == 0 for at, _ in regions) and regions[0][0] == 0
        assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:])) and regions[-1][0] + regions[-1][1] <= arena
    print(f"resnet50 at 480 x 640: {macs / 1e9:.2f} GMAC per frame")
    for _ in bad:
        assert next(out) == "0"
    for cout, cin, k, a, want in records:
        got = next(out).split()
        assert int(got[0]) == int(want), (cout, cin, k, sorted(a))
        if not want:
            assert len(got) == 1
            continue
        words = np.array([int(v, 16) for v in got[1:]], np.uint32)
        K = k * k * cin
        assert len(words) == K * cout + 2 * cout
        relaid = a["weight"].transpose(2, 3, 1, 0).reshape(K, cout)
        assert np.array_equal(words[:K * cout], np.ascontiguousarray(relaid).ravel().view(np.uint32))
        w = {"bn." + n: v for n, v in (("weight", a["bn_weight"]), ("bias", a["bn_bias"]), ("running_mean", a["running_mean"]), ("running_var", a["running_var"]))}
        scale, shift = R.fold(w, "bn", eps, np.float32)
        assert np.array_equal(words[K * cout:K * cout + cout], scale.view(np.uint32)) and np.array_equal(words[K * cout + cout:], shift.view(np.uint32))
    assert next(out, None) is None
