"""Writes tests/golden/vos/vos_reference.npz: inputs and the reference's own results for them.

    python tests/golden/make_vos_golden.py          (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/vos_ref.py)

The reference's transductive-vos.pytorch/lib/predict.py is loaded by path under two shims (np.int, an identity Tensor.cuda) and its
predict, sample_frames and get_spatial_weight are called as run_video.py calls them, on CPU torch.  idx2onehot names a CUDA device,
so its one scatter is restated (vos_ref.onehot).  Only inputs and results are stored:
  per group of vos_ref.GROUPS  a history of frames (features as int8 levels and one fp32 multiplier, labels), and per frame_idx of
                               the group the reference's fp32 prediction; the first group runs 1, 3, 9, 10, 15, 16, 17, 24, 60 over 60 frames
  tol_<group>                  4 x err_ref, err_ref = max |pred_ref32 - pred_64| / max_c |pred_64[:, q]| over the group's cases
  sample_<ref_num>_<range>     the reference's sample_frames for frame_idx 1 .. 300, -1 padded
  interp_*                     torch's interpolate(mode='bilinear', align_corners=False) on the CPU, both directions
The file is written only if the reference's own fp32 result is inside its group's bar and decision rule against fp64."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vos_ref as V  # noqa: E402

INTERP_SIZES = ((52, 68), (64, 64), (8, 8))


def main():
    ref = V.reference_module()
    if ref is None:
        raise SystemExit(f"no reference checkout at {V.reference_dir()}")
    import torch
    args = types.SimpleNamespace(range=V.DEFAULTS["range"], ref_num=V.DEFAULTS["ref_num"], temperature=V.DEFAULTS["temperature"])
    out = {}
    left_out = total = 0
    for g, (name, Hd, Wd, H, W, C, d, scale, idxs) in enumerate(V.GROUPS):
        q, mult, labels = V.make_history(20260 + g, Hd, Wd, H, W, C, d, max(idxs) + 1, scale)
        feats = V.features(q, mult)
        w_dense = ref.get_spatial_weight((Hd, Wd), V.DEFAULTS["sigma_dense"])
        w_sparse = ref.get_spatial_weight((Hd, Wd), V.DEFAULTS["sigma_sparse"])
        out[f"{name}_q"], out[f"{name}_mult"], out[f"{name}_labels"] = q, mult, labels
        errs, preds, logit_max = [], [], 0.0
        for f in idxs:
            hist = torch.from_numpy(feats[:f]).reshape(f, C, Hd, Wd)
            lab = torch.from_numpy(np.ascontiguousarray(labels[:f].transpose(1, 0, 2)))          # (d, N, HW) as run_video.py keeps it
            with torch.no_grad():
                pred = ref.predict(hist, torch.from_numpy(feats[f]).reshape(C, Hd, Wd), lab, w_dense, w_sparse, f, args).numpy()
            sel, n_dense = V.sample_frames(f)
            assert sel == ref.sample_frames(f, args.range, args.ref_num).tolist()
            p64 = V.predict(feats[sel], labels[sel], feats[f], n_dense, Hd, Wd)
            logit_max = max(logit_max, float(np.abs(np.einsum("ncp,cq->npq", feats[sel].astype(np.float64), feats[f])).max()))
            errs.append(V.rel_err(pred, p64))
            preds.append(pred)
        tol = 4.0 * max(errs)
        for f, pred in zip(idxs, preds):
            sel, n_dense = V.sample_frames(f)
            p64 = V.predict(feats[sel], labels[sel], feats[f], n_dense, Hd, Wd)
            err, ok = V.check(pred, p64, tol)
            assert ok, (name, f, err, tol)
            left_out += V.decisions_ok(np.argmax(pred, 0), p64, tol)[1]
            total += p64.shape[1]
        out[f"{name}_pred"] = np.stack(preds)
        out[f"tol_{name}"] = np.float64(tol)
        print(f"{name}: {len(idxs)} cases, |logit| up to {logit_max:.1f}, err_ref {max(errs):.3e}, tol {tol:.3e}")
    print(f"{left_out} of {total} positions under the margin")
    for ref_num, rng in V.SAMPLE_CONFIGS:
        tab = np.full((300, ref_num), -1, np.int32)
        for f in range(1, 301):
            sel = ref.sample_frames(f, rng, ref_num).tolist()
            tab[f - 1, :len(sel)] = sel
        out[f"sample_{ref_num}_{rng}"] = tab
    rs = np.random.default_rng(20269)
    for H, W in INTERP_SIZES:
        Hd, Wd = V.grid_of(H, W)
        lab = V.label_image(H, W, 3, 1, seed=H)
        down = torch.nn.functional.interpolate(torch.from_numpy(V.onehot(lab, 3))[None], size=(Hd, Wd), mode="bilinear", align_corners=False)[0].numpy()
        pred = rs.random((3, Hd, Wd), dtype=np.float32)
        up = torch.nn.functional.interpolate(torch.from_numpy(pred)[None], size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
        out[f"interp_{H}x{W}_label"], out[f"interp_{H}x{W}_down"], out[f"interp_{H}x{W}_pred"], out[f"interp_{H}x{W}_up"] = lab, down, pred, up
    os.makedirs(os.path.dirname(V.GOLDEN), exist_ok=True)
    np.savez_compressed(V.GOLDEN, **out)
    print(V.GOLDEN, os.path.getsize(V.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
