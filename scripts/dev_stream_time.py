"""Dev: the feature manager on device-resident tables at throughput size - 4096 windows of about 150 rows, 120-point images.

Reports the kernel times of one frame's bookkeeping (avm_last_kernel_ms: imu_push, add_image, solve_view, store_depths, slide_window)
and, in the same run, the time of copying the track tables device -> host -> device: the floor of any bookkeeping done by the host, the
thing these calls replace.  Not a test.  Usage: python scripts/dev_stream_time.py [n_windows]
"""
import importlib
import json
import statistics
import sys
import time

import numpy as np

sys.path[:0] = ["."]
PKG = "anticipated-vins-mono_amd"
mod = lambda n: importlib.import_module(PKG + "." + n)
abi, buffers = mod("abi"), mod("buffers")

MAX_FEAT, MAX_OBS, MAX_SAMP, MAX_PTS = 256, 2816, 40, 128
ROWS, POINTS, MATCHED = 150, 120, 90
COPIED = ("n_feat", "feat_start", "feat_nobs", "feat_obs_begin", "obs_xy", "inv_depth")   # + feat_id: what a host's bookkeeping reads and rewrites


def build_base(B=8, seed=1):
    """B windows as a frame's loop finds them (observations up to frame 9, interval 9 empty), their ids and one image each"""
    rng = np.random.default_rng(seed)
    a = {"pose": np.zeros((B, 11, 7)), "speedbias": np.zeros((B, 11, 9)), "ex_pose": np.zeros((B, 7)), "inv_depth": np.zeros((B, MAX_FEAT)),
         "n_feat": np.full(B, ROWS, np.int32), "feat_start": np.zeros((B, MAX_FEAT), np.int32), "feat_nobs": np.zeros((B, MAX_FEAT), np.int32),
         "feat_obs_begin": np.zeros((B, MAX_FEAT), np.int32), "obs_xy": np.zeros((B, MAX_OBS, 2)), "imu_n": np.full((B, 10), 20, np.int32),
         "imu_dt": np.full((B, 10, MAX_SAMP), 0.005), "imu_acc": np.zeros((B, 10, MAX_SAMP + 1, 3)), "imu_gyr": np.zeros((B, 10, MAX_SAMP + 1, 3)),
         "imu_lin_ba": np.zeros((B, 10, 3)), "imu_lin_bg": np.zeros((B, 10, 3))}
    a["pose"][:, :, 6], a["ex_pose"][:, 6] = 1.0, 1.0
    a["pose"][:, :, :3] = rng.normal(scale=0.1, size=(B, 11, 3))
    a["imu_acc"][..., 2], a["imu_n"][:, 9] = 9.81, 0
    fid = np.full((B, MAX_FEAT), -1, np.int32)
    img = {"n_pts": np.full(B, POINTS, np.int32), "feature_id": np.zeros((B, MAX_PTS), np.int32), "xy": rng.normal(scale=0.3, size=(B, MAX_PTS, 2))}
    for b in range(B):
        start = np.sort(np.r_[rng.integers(0, 8, 120), rng.integers(8, 10, ROWS - 120)])
        alive = rng.permutation(ROWS)[:MATCHED + 15]                                   # tracks that reach frame 9
        nobs = np.array([rng.integers(3 if s == 0 else 1, 10 - s + 1) for s in start])
        nobs[alive] = 10 - start[alive]
        a["feat_start"][b, :ROWS], a["feat_nobs"][b, :ROWS] = start, nobs
        a["feat_obs_begin"][b, :ROWS] = np.r_[0, np.cumsum(nobs)[:-1]]
        a["obs_xy"][b, :nobs.sum()] = rng.normal(scale=0.3, size=(nobs.sum(), 2))
        a["inv_depth"][b, :ROWS] = rng.uniform(0.1, 0.5, ROWS)
        fid[b, :ROWS] = rng.permutation(4 * ROWS)[:ROWS] * 2 + 1
        ids = np.r_[fid[b, alive[:MATCHED]], rng.permutation(4 * ROWS)[:POINTS - MATCHED] * 2]
        img["feature_id"][b, :POINTS] = np.sort(ids)
    dims = dict(n_windows=B, max_feat=MAX_FEAT, max_obs=MAX_OBS, max_samp=MAX_SAMP, max_prior=96, max_pblk=16)
    return buffers.WindowArrays(dims, a), fid, buffers.ImageArrays({"n_windows": B, "max_pts": MAX_PTS}, img)


def tile(x, n):
    return np.ascontiguousarray(np.concatenate([x] * (n // x.shape[0] + 1))[:n])


def main(n_windows):
    import torch

    ctx = mod("lib").Context(0)
    E = mod("estimator").Estimator(ctx=ctx, options=abi.default_options())
    w, fid, img = build_base()
    d = dict(w.dims)
    d["n_windows"] = n_windows
    dev = "cuda:0"
    full0 = buffers.WindowArrays(d, {k: tile(v, n_windows) for k, v in w.a.items()}).to_device(dev)
    fid0 = torch.from_numpy(tile(fid, n_windows)).to(dev)
    image = buffers.ImageArrays({"n_windows": n_windows, "max_pts": MAX_PTS}, {k: tile(v, n_windows) for k, v in img.a.items()}).to_device(dev)
    n = torch.full((n_windows,), 20, dtype=torch.int32, device=dev)
    dt = torch.full((n_windows, 20), 0.005, dtype=torch.float64, device=dev)
    acc = torch.zeros((n_windows, 20, 3), dtype=torch.float64, device=dev)
    acc[..., 2] = 9.81
    flags = torch.from_numpy(tile(np.array([abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW], np.int32), n_windows)).to(dev)
    ms = {k: [] for k in ("imu_push", "add_image", "solve_view", "store_depths", "slide_window")}
    copies = []
    for rep in range(7):
        T = buffers.TrackTables(full0.copy(), fid0.clone())
        E.push_imu(T.full, n, dt, acc, acc)
        E.addFeatureCheckParallax(T.full, T.feat_id, image, 10.0 / 460.0)
        E.solve_view(T)
        E.setDepth(T)
        E.slideWindow(T.full, flags, True, 5.0, remove_failures=True, feat_id=T.feat_id)
        for k in ms:
            ms[k].append(ctx.kernel_ms(k))
        # the copy a host's bookkeeping cannot avoid: the track tables to the host and back
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [T.full.a[k].cpu() for k in COPIED] + [T.feat_id.cpu()]
        for src, k in zip(host, COPIED):
            T.full.a[k].copy_(src)
        T.feat_id.copy_(host[-1])
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    out = {"n_windows": n_windows, "rows": ROWS, "image_points": POINTS, "rows_after": int(T.full.a["n_feat"].max()),
           "kernel_ms_median": {k: round(statistics.median(v[2:]), 4) for k, v in ms.items()},
           "copy_d2h_h2d_ms_median": round(statistics.median(copies[2:]), 3),
           "copied_mib": round(sum(T.full.a[k].numel() * T.full.a[k].element_size() for k in COPIED) / 2**20 + T.feat_id.numel() * 4 / 2**20, 1)}
    out["kernel_ms_sum"] = round(sum(out["kernel_ms_median"].values()), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096)
