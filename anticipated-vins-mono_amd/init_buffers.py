"""Caller-owned buffers behind the structs of include/avm_init.h, the initialisation phase (buffers.py holds those of include/avm.h)."""
import numpy as np

from . import abi, buffers


class SfmBatchArrays(buffers.SfmArrays):
    """avm_sfm_batch: buffers.SfmArrays (what synth.make_sfm returns) with the struct avm_global_sfm_batch takes."""

    STRUCT = abi.SfmBatch

    @staticmethod
    def of(sfm: buffers.SfmArrays) -> "SfmBatchArrays":
        """the same arrays (no copy) behind the struct"""
        return sfm if isinstance(sfm, SfmBatchArrays) else SfmBatchArrays(sfm.dims, sfm.a)


class SfmOutArrays(buffers._Arrays):
    """avm_sfm_out: ok [B], frame_R [B, max_frames, 9], frame_T [B, max_frames, 3], q [B, 11, 4] (w x y z), T [B, 11, 3],
    point [B, max_feat, 3], point_state [B, max_feat], ba_counts [B, 3], ba_cost [B, 2] and, with want_chain, pnp_q / pnp_t.  A stream
    writes only the rows its ok allows (include/avm_init.h): alloc() gives zeros, `fill` another sentinel for the doubles."""

    STRUCT, PER_STREAM = abi.SfmOut, "ok"

    @staticmethod
    def alloc(n_windows: int, max_frames: int, max_feat: int, device=None, want_chain: bool = True, fill: float = 0.0) -> "SfmOutArrays":
        B, K = n_windows, abi.NFRAMES
        a = {"ok": np.zeros(B, np.int32), "frame_R": np.full((B, max_frames, 9), fill), "frame_T": np.full((B, max_frames, 3), fill),
             "q": np.full((B, K, 4), fill), "T": np.full((B, K, 3), fill), "point": np.full((B, max_feat, 3), fill),
             "point_state": np.zeros((B, max_feat), np.int32), "ba_counts": np.zeros((B, 3), np.int32), "ba_cost": np.full((B, 2), fill)}
        if want_chain:
            a["pnp_q"], a["pnp_t"] = np.full((B, K, 4), fill), np.full((B, K, 3), fill)
        o = SfmOutArrays({}, a)
        return o.to_device(device) if device else o
