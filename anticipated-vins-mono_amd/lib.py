"""Loader for the product library libavm_hip.so (HIP/gfx950).  No fallback: a missing library
or a missing GPU raises, it never silently routes to CPU code."""
import ctypes as C
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libavm_hip.so")
_lib = None


class AvmError(RuntimeError):
    pass


def build(force: bool = False):
    """Compile csrc/*.hip for gfx950 with hipcc (works without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise AvmError(
                f"{_LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        # PyTorch-ROCm ships its own copy of the HIP / HSA runtime under the same sonames.  Whichever is loaded first serves
        # the whole process, and torch cannot find the GPU on top of /opt/rocm's: load torch's first when it is installed,
        # so that `import torch` after this module keeps working (device tensors are how the tests and bench.py hand over
        # HBM-resident buffers).  A C++ host (include/avm_host.hpp) has no such concern.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIB_PATH)
        for table in (abi.PROTOTYPES, abi.PROTOTYPES_INIT):
            for name, (restype, argtypes) in table.items():
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


# the functions include/avm.h declares: __graft_entry__.build() looks every one up
EXPORTS = [name for name in abi.PROTOTYPES if not name.startswith("avm_debug_")]
# ... and the ones of include/avm_init.h
EXPORTS_INIT = list(abi.PROTOTYPES_INIT)


class Context:
    """avm_ctx: one per host thread, owns device scratch and one HIP stream."""

    def __init__(self, device: int = 0):
        self._L = lib()
        cfg = abi.Config()
        cfg.device = device
        cfg.abi_version = abi.AVM_ABI_VERSION
        h = C.c_void_p()
        rc = self._L.avm_create(C.byref(cfg), C.byref(h))
        if rc != abi.AVM_OK:
            raise AvmError(f"avm_create failed with status {rc} (no HIP device? there is no CPU fallback)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self._L.avm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str):
        if rc != abi.AVM_OK:
            raise AvmError(f"{what} failed: status {rc}: {self._L.avm_last_error(self.h).decode()}")

    def call(self, name: str, *args):
        """The entry point `name` on this ctx (the handle goes first); a status other than AVM_OK raises AvmError with the library's message."""
        self.check(getattr(self._L, name)(self.h, *args), name)

    @property
    def device_str(self) -> str:
        """the torch name of this ctx's device"""
        return "cuda:%d" % self.device

    def _int64s(self, name: str, n: int) -> list:
        """the n counters the hook `name` writes"""
        out = (C.c_int64 * n)()
        self.call(name, out)
        return [int(v) for v in out]

    # ---- multi-GPU: the library's own RCCL communicator (include/avm.h)
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self.call("avm_comm_unique_id", buf)
        return buf.raw

    def comm_init(self, n_ranks: int, rank: int, uid: bytes):
        assert len(uid) == 128
        self.call("avm_comm_init", int(n_ranks), int(rank), C.create_string_buffer(uid, 128))

    def gather_states(self, send, recv, count: int):
        """ncclAllGather of `count` doubles per rank (device tensors): recv[r * count : (r + 1) * count] = rank r's send."""
        self.call("avm_gather_states", abi.dptr(send), abi.dptr(recv), int(count))

    def comm_destroy(self):
        self.call("avm_comm_destroy")

    def fsel_fallback_stats(self) -> dict:
        """avm_fsel_fallback_stats: how often this ctx's selects fell back from the all-rounds-in-one-launch kernel."""
        return dict(zip(("reruns", "failed_launches", "mode", "calls"), self._int64s("avm_fsel_fallback_stats", 4)))

    def last_solve_form(self) -> str:
        """Which form of the solve kernel the last optimization() took: 'throughput' (two 256-thread workgroups per CU,
        batches larger than the CU count) or 'latency' (one 512-thread workgroup per CU).  AVM_SOLVE_TP=0/1 forces it."""
        return "throughput" if self._L.avm_debug_last_solve_form(self.h) == 1 else "latency"

    def last_marg_form(self) -> str:
        """Which form of the marginalization kernel the last optimization() took: 'throughput' (two 256-thread workgroups per CU; it
        follows the solve's form unless a prior keeps a speed-bias block beyond frame 1, AVM_MARG_TP=0 switches it off) or 'latency'."""
        return "throughput" if self._L.avm_debug_last_marg_form(self.h) == 1 else "latency"

    def last_split(self) -> tuple:
        """How the last optimization() split its batch (avm_window_solve_batch_relo): (windows solved as plain ones, windows that took the
        extended kernel, the plain ones' form: 0 latency / 1 throughput / -1 there were none, 1 when the list builds of the kernels ran)."""
        return tuple(self._int64s("avm_debug_last_split", 4))

    def last_fsel_form(self) -> str:
        """Which form the last select_batch() started in: 'solo' (one workgroup per frame with lazy evaluation: batches of 33 frames and
        more; AVM_FSEL_SOLO=0/1 forces it), 'teams' (a team of workgroups per frame) or 'rounds' (one launch per round)."""
        return {3: "solo", 2: "teams", 1: "teams", 0: "rounds"}.get(self._L.avm_debug_last_fsel_form(self.h), "none")

    def last_fsel_evaluations(self) -> int:
        """Candidate evaluations the last select_batch() executed on the device: counted by the solo form's kernel (lazy evaluation);
        -1 for the forms that score every live candidate in every round (their count follows from the frame: bench.py)."""
        return self._int64s("avm_debug_fsel_evaluations", 1)[0]

    def counters(self) -> dict:
        """Debug counters of this ctx: device / pinned (re)allocations so far, and how the last marginalization's square roots were taken."""
        allocs, one_wave, windows, tp = self._int64s("avm_debug_counters", 4)
        return {"allocations": allocs, "prior_one_wavefront": one_wave, "prior_windows": windows, "prior_pivoted_path": windows - one_wave,
                "solve_form": "throughput" if tp else "latency"}

    def preint_cache(self) -> dict:
        """The ctx's pre-integration cache: intervals the last pre-integration examined and how many of them it integrated (the ones
        whose IMU samples or linearization biases differ from what the stored results came from; all of them with AVM_PREINT_CACHE=0),
        and the windows whose cached intervals the last slide_window rolled (0: it left the cache alone)."""
        return dict(zip(("examined", "recomputed", "rolled_windows"), self._int64s("avm_debug_preint_cache", 3)))

    def kernel_ms(self, which: str) -> float:
        ms = C.c_float(0)
        self.call("avm_last_kernel_ms", which.encode(), C.byref(ms))
        return ms.value

