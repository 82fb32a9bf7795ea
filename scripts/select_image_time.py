"""The selector in the stream loop at throughput size: 4096 windows (tiled from 32 distinct ones), images of 200 points - 50 tracked plus
150 new -, max_features 150, horizon 10, everything device-resident.

Reports the kernel times of avm_fsel_select_image_batch (avm_last_kernel_ms: select_split, select_merge, fsel_select; the last four of
five calls) and, on the same data, the path it replaces: image and state device -> host, FeatureSelector.select's bookkeeping per window on
dicts and lists, the problem arrays host -> device, the same avm_fsel_select_batch, the ids device -> host, the rebuilt images host ->
device.  Not a test.  Usage: python scripts/select_image_time.py [n_windows] [--md profiles/select_image.md]
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
abi, buffers, synth = mod("abi"), mod("buffers"), mod("synth")

DISTINCT, TRACKED, NEW, MAXF, HORIZON = 32, 50, 150, 150, 10
POINTS = TRACKED + NEW


def tile(x, n):
    return np.ascontiguousarray(np.concatenate([x] * (n // x.shape[0] + 1))[:n])


def build(n_windows):
    """(image with prob, state, problem) on the host: make_fsel's used points are the tracked ones, its candidates the new ones"""
    f = synth.make_fsel(DISTINCT, horizon=HORIZON, n_cand=NEW, n_used=TRACKED, n_cloud=150, max_features=MAXF)
    rng = np.random.default_rng(2)
    img = {"n_pts": np.full(DISTINCT, POINTS, np.int32), "feature_id": np.concatenate([f.a["used_id"], f.a["cand_id"]], 1),
           "xy": np.concatenate([f.a["used_xy"], f.a["cand_xy"]], 1),
           "prob": np.concatenate([rng.uniform(0.05, 1.0, (DISTINCT, TRACKED)).astype(np.float32).astype(np.float64), f.a["cand_prob"]], 1)}
    st = buffers.SelectorState.alloc(DISTINCT, 256)
    st.a["last_feature_id"][:], st.a["n_tracked"][:], st.a["first_image"][:] = f.a["used_id"][:, -1], TRACKED, 0
    for b in range(DISTINCT):
        st.a["tracked_id"][b, :TRACKED] = rng.permutation(f.a["used_id"][b])
    image = buffers.ImageArrays({"n_windows": n_windows, "max_pts": POINTS}, {k: tile(v, n_windows) for k, v in img.items()})
    state = buffers.SelectorState(st.dims, {k: tile(v, n_windows) for k, v in st.a.items()})
    d = dict(f.dims)
    d["n_problems"] = n_windows
    return image, state, buffers.FselArrays(d, {k: tile(v, n_windows) for k, v in f.a.items()}, f.scalars)


def host_path(sel, image, state, problem, torch):
    """one frame through the host: returns the milliseconds of every step"""
    ms, t = {}, time.perf_counter()

    def lap(key):
        nonlocal t
        torch.cuda.synchronize()
        now = time.perf_counter()
        ms[key], t = (now - t) * 1e3, now

    torch.cuda.synchronize()
    t = time.perf_counter()
    hi, hs = image.to_host(), state.to_host()
    lap("d2h_image_state")
    B = image.n_windows
    pa = {k: np.zeros(tuple(problem.a[k].shape), np.int32 if k in ("n_cand", "cand_id", "n_used", "used_id") else np.float64)
          for k in ("n_cand", "cand_id", "cand_xy", "cand_prob", "n_used", "used_id", "used_xy")}
    images, subsets = [], []
    for b in range(B):                                                      # splitOnFeatureId and the tracked-feature lookup, as FeatureSelector.select does them
        n = int(hi.a["n_pts"][b])
        im = {int(i): (xy, p) for i, xy, p in zip(hi.a["feature_id"][b, :n], hi.a["xy"][b, :n], hi.a["prob"][b, :n])}
        last = int(hs.a["last_feature_id"][b])
        ids = sorted(im)
        new = [i for i in ids if i > last]
        old = {i: im[i] for i in ids if i <= last}
        if new:
            hs.a["last_feature_id"][b] = new[-1]
        subset = {f: old[f] for f in hs.a["tracked_id"][b, :int(hs.a["n_tracked"][b])].tolist() if f in old}
        used = sorted(subset)
        pa["n_cand"][b], pa["n_used"][b] = len(new), len(used)
        pa["cand_id"][b, :len(new)], pa["used_id"][b, :len(used)] = new, used
        for j, i in enumerate(new):
            pa["cand_xy"][b, j], pa["cand_prob"][b, j] = im[i]
        for j, i in enumerate(used):
            pa["used_xy"][b, j] = im[i][0]
        images.append(im), subsets.append(subset)
    lap("bookkeeping_split")
    for k, v in pa.items():
        problem.a[k].copy_(torch.from_numpy(v))
    lap("h2d_problem")
    out = sel.select_batch(problem, want_fvalues=False)
    lap("select_batch_call")
    ms["fsel_select_kernels"] = sel.ctx.kernel_ms("fsel_select")
    nsel, ids = out.a["n_selected"].cpu().numpy(), out.a["selected_ids"].cpu().numpy()
    lap("d2h_ids")
    io = {"n_pts": np.zeros(B, np.int32), "feature_id": np.zeros((B, POINTS), np.int32), "xy": np.zeros((B, POINTS, 2))}
    for b in range(B):                                                      # image.swap(subset) and the tracked list
        picked = ids[b, :nsel[b]].tolist()
        for f in picked:
            subsets[b][f] = images[b][f]
        keys = sorted(subsets[b])
        io["n_pts"][b] = len(keys)
        io["feature_id"][b, :len(keys)] = keys
        for j, i in enumerate(keys):
            io["xy"][b, j] = subsets[b][i][0]
        nt = int(hs.a["n_tracked"][b])
        hs.a["tracked_id"][b, nt:nt + len(picked)] = picked
        hs.a["n_tracked"][b] = nt + len(picked)
    lap("bookkeeping_merge")
    dev = [torch.from_numpy(v).to("cuda:0") for v in io.values()] + [torch.from_numpy(v).to("cuda:0") for v in hs.a.values()]
    lap("h2d_image_state")
    return ms, int(nsel.sum())


def main(n_windows, md):
    import torch

    ctx = mod("lib").Context(0)
    sel = mod("feature_selector").FeatureSelector(ctx=ctx)
    image, state0, problem = (x.to_device("cuda:0") for x in build(n_windows))
    keys = ("select_split", "select_merge", "fsel_select")
    ms, n_out = {k: [] for k in keys}, 0
    for rep in range(5):
        state = state0.copy()
        out, image_out = sel.select_stream(image, state, problem, None, 0, True)
        for k in keys:
            ms[k].append(ctx.kernel_ms(k))
        n_out = int(image_out.a["n_pts"].sum())
    selected = int(out.a["n_selected"].sum())
    host_ms, host_selected = host_path(sel, image, state0.copy(), problem, torch)
    res = {"n_windows": n_windows, "distinct": DISTINCT, "image_points": POINTS, "tracked": TRACKED, "new": NEW, "max_features": MAXF, "horizon": HORIZON,
           "form": ctx.last_fsel_form(), "selected": selected, "image_out_points": n_out,
           "kernel_ms_median_last4": {k: round(statistics.median(v[1:]), 4) for k, v in ms.items()},
           "kernel_ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "host_path_ms": {k: round(v, 3) for k, v in host_ms.items()}, "host_path_selected": host_selected}
    k = res["kernel_ms_median_last4"]
    res["device_bookkeeping_ms"] = round(k["select_split"] + k["select_merge"], 4)
    res["host_bookkeeping_and_copies_ms"] = round(sum(v for n, v in host_ms.items() if n not in ("select_batch_call", "fsel_select_kernels")), 3)
    print(json.dumps(res), flush=True)
    if md:
        with open(md, "w") as f:
            f.write("# The selector in the stream loop: avm_fsel_select_image_batch against the host path it replaces\n\n")
            f.write("Generated by `scripts/select_image_time.py %d` on an MI355X.  %d windows tiled from %d distinct ones, images of %d points (%d tracked, %d new), "
                    "max_features %d, horizon %d, device-resident; the selection takes the %s form and picks %d ids in all.\n\n"
                    % (n_windows, n_windows, DISTINCT, POINTS, TRACKED, NEW, MAXF, HORIZON, res["form"], selected))
            f.write("## Device (avm_last_kernel_ms, median of the last four of five calls)\n\n| key | ms |\n|---|---|\n")
            for n in keys:
                f.write("| %s | %.4f |\n" % (n, k[n]))
            f.write("| select_split + select_merge | %.4f |\n\n" % res["device_bookkeeping_ms"])
            f.write("## The host path on the same data (one frame, wall clock)\n\n| step | ms |\n|---|---|\n")
            for n, v in res["host_path_ms"].items():
                f.write("| %s | %.3f |\n" % (n, v))
            f.write("| everything but the selection | %.3f |\n\n" % res["host_bookkeeping_and_copies_ms"])
            f.write("`select_batch_call` is the wall clock of the same avm_fsel_select_batch, `fsel_select_kernels` its device time: the selection is not what "
                    "the new call changes.  The host path selected %d ids.\n" % host_selected)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--md" and not a.endswith(".md")]
    mds = [a for a in sys.argv[1:] if a.endswith(".md")]
    main(int(args[0]) if args else 4096, mds[0] if mds else None)
