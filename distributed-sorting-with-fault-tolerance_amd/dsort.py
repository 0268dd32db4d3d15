"""ctypes binding of libdsort (include/dsort.h) for tests, the bench and __graft_entry__.

The product is the C ABI in lib/libdsort.so (HIP kernels for gfx950); this module only loads it
and converts arguments.  There is no fallback: if the library is missing or no gfx950 device is
present, the calls raise.  torch is imported BEFORE the library so that libdsort binds to the HIP
runtime torch already loaded (same soname libamdhip64.so.7): device memory from torch tensors and
the library's kernels then live in one runtime.
"""
import contextlib
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# DSORT_LIB: an alternative build of the same library (A/B experiments of compile-time variants)
LIB_PATH = os.environ.get("DSORT_LIB") or os.path.join(HERE, "lib", "libdsort.so")

try:  # shared HIP runtime (see module docstring); absence of torch is fine on the CPU box
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

DSORT_OK = 0
DSORT_ECOMM = -4
DSORT_ETIMEOUT = -6
ERRORS = {-1: "EINVAL", -2: "ENOMEM", -3: "EHIP", -4: "ECOMM", -5: "ENODEV", -6: "ETIMEOUT", -7: "ESTAGE"}

# every symbol include/dsort.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "dsort_init", "dsort_finalize", "dsort_last_error", "dsort_version", "dsort_get_stats",
    "dsort_synchronize", "dsort_set_option", "dsort_get_option", "dsort_sort_stages", "dsort_sample_sort_stages", "dsort_sort_i32", "dsort_sort_i64", "dsort_sort_dev_i32",
    "dsort_sort_dev_i64", "dsort_sort_dev_copy_i32", "dsort_sort_dev_copy_i64",
    "dsort_merge_i32", "dsort_merge_i64", "dsort_merge_dev_i32", "dsort_merge_dev_i64",
    "dsort_comm_unique_id", "dsort_comm_init", "dsort_comm_init_transport", "dsort_comm_abort",
    "dsort_comm_destroy", "dsort_comm_deadline_ms",
    "dsort_sample_sort_dev_i32", "dsort_sample_sort_dev_i64", "dsort_sample_merge_dev_i32",
    "dsort_sample_merge_dev_i64", "dsort_plan_splitters_i32",
    "dsort_plan_splitters_i64", "dsort_plan_cuts_i32", "dsort_plan_cuts_i64",
    "dsort_plan_sample_positions", "dsort_gen_uniform_i32", "dsort_gen_uniform_i64",
    "dsort_gen_zipf_i64", "dsort_fingerprint_i32", "dsort_fingerprint_i64",
    "dsort_count_descents_i32", "dsort_count_descents_i64", "dsort_dev_alloc", "dsort_dev_free",
    "dsort_copy_h2d", "dsort_copy_d2h", "dsort_copy_d2d", "dsort_host_register",
    "dsort_host_unregister", "dsort_write_text_i32", "dsort_format_text_dev_i32",
    "dsort_parse_text_dev_i32", "dsort_parse_text_i32", "dsort_format_text_i32",
    "dsort_argsort_dev_i32", "dsort_sort_pairs_dev_i32", "dsort_gather_dev", "dsort_argsort_i32",
    "dsort_sample_argsort_dev_i32", "dsort_sample_sort_pairs_dev_i32",
    "dsort_sample_gather_dev", "dsort_plan_gather_table", "dsort_plan_gather_route",
    "dsort_argsort_dev_i64", "dsort_argsort_i64", "dsort_sort_records_dev_i64", "dsort_plan_argsort_i64",
    "dsort_sample_argsort_dev_i64", "dsort_plan_sample_argsort_i64",
    # typed keys and descending order (an ABI 10 addition)
    "dsort_key_encode", "dsort_key_decode", "dsort_sort_dev_keys", "dsort_sort_dev_copy_keys",
    "dsort_sort_keys", "dsort_argsort_dev_keys", "dsort_argsort_keys", "dsort_sort_pairs_dev_keys",
    "dsort_sort_records_dev_keys", "dsort_sample_sort_dev_keys", "dsort_sample_argsort_dev_keys",
    # top-k selection (an ABI 10 addition)
    "dsort_plan_topk", "dsort_topk_dev_keys", "dsort_topk_keys", "dsort_sample_topk_dev_keys",
]

# DSORT_KEY_* and DSORT_ORDER_DESCENDING (include/dsort.h, "Key types and order")
KEY_TYPES = {"i32": 0, "u32": 1, "f32": 2, "i64": 3, "u64": 4, "f64": 5}
ORDER_DESCENDING = 1
_KEY_OF_NP = {np.dtype(np.int32): "i32", np.dtype(np.uint32): "u32", np.dtype(np.float32): "f32",
              np.dtype(np.int64): "i64", np.dtype(np.uint64): "u64", np.dtype(np.float64): "f64"}
_NP_OF_KEY = {v: k for k, v in _KEY_OF_NP.items()}


# dsort_set_option / dsort_get_option (include/dsort.h)
OPTIONS = {"buckets": 1, "bucket_keys": 2, "bucket_oversample": 3,
           "max_fanin_log2": 5, "kill_after_stage": 6, "kill_in_exchange": 7,
           "comm_timeout_ms": 8,
           "sub_keys": 9, "sub_oversample": 10, "sub_gather": 11, "test_hold_exchange": 12,
           "test_fail_exchange": 13, "stage_timing": 14, "test_tile_cap": 15,
           "test_wave_fence": 16, "argsort_wide": 17, "test_fail_leg": 18, "topk_path": 19}


class DsortError(RuntimeError):
    pass


class Stats(ctypes.Structure):
    _fields_ = [("block_sort_ms", ctypes.c_double), ("merge_ms", ctypes.c_double),
                ("exchange_ms", ctypes.c_double), ("final_merge_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("merge_kernel_ms", ctypes.c_double),
                ("merge_kernel_launches", ctypes.c_int), ("merge_passes", ctypes.c_int),
                ("tile_keys", ctypes.c_int), ("keys_in", ctypes.c_size_t),
                ("keys_out", ctypes.c_size_t), ("alltoall_ms", ctypes.c_double),
                ("keys_sent", ctypes.c_size_t), ("tile_sort_kernel_ms", ctypes.c_double),
                ("partition_ms", ctypes.c_double), ("tile_sort_keys", ctypes.c_size_t),
                ("bucket_hist_ms", ctypes.c_double), ("bucket_scatter_ms", ctypes.c_double),
                ("sub_partition_ms", ctypes.c_double), ("sub_split_subbuckets", ctypes.c_int),
                ("sub_scatter_fallback", ctypes.c_int), ("exchange_path", ctypes.c_int),
                ("first_level_map", ctypes.c_int),
                ("fence_ranges", ctypes.c_int),  # ABI 6
                ("deferred_frees", ctypes.c_int), ("pending_frees", ctypes.c_int),
                ("argsort_passes", ctypes.c_int),  # ABI 10, in what was padding
                ("gather_sent", ctypes.c_size_t), ("gather_served", ctypes.c_size_t)]  # ABI 9

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_size_t)
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
                                ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                                ctypes.POINTER(ctypes.c_size_t))


class Transport(ctypes.Structure):
    """dsort_transport: the sample sort's exchanges through host callbacks (dsort.h)."""
    _fields_ = [("user", ctypes.c_void_p), ("allgather", ALLGATHER_FN), ("alltoallv", ALLTOALLV_FN)]


def torch_dist_transport(world, pg=None, deadline_fn=None):
    """A dsort_transport over a torch.distributed process group (gloo: CPU tensors; the default
    group unless `pg` is given).  For ranks that share a GPU, where RCCL refuses to build a
    communicator, and for the survivors' group after a fault (ftsort.py).

    Every wait is bounded by the exchange deadline: `deadline_fn()` gives the milliseconds left
    (-1 = none).  Context.comm_init_transport sets it to dsort_comm_deadline_ms, so a collective
    whose peer never arrives returns DSORT_ETIMEOUT (-6) at the sort's DSORT_OPT_COMM_TIMEOUT_MS
    instead of blocking until gloo's own timeout (dsort.h, ABI 5).

    A timed-out gloo operation stays queued on the group, so a later collective on it could pair
    with a slow peer's stale one (a status gate and a key count are both 8 bytes).  After the first
    timeout the transport is therefore POISONED: every later callback fails at once (the sort
    returns DSORT_ECOMM) and the group must be rebuilt, as ftsort.py does for its survivors."""
    import datetime

    import torch.distributed as dist

    def _wait(work):
        fn = t.deadline_fn
        ms = fn() if fn is not None else -1
        if ms is None or ms < 0:
            work.wait()
            return 0
        try:
            work.wait(timeout=datetime.timedelta(milliseconds=max(int(ms), 1)))
        except RuntimeError as e:
            if "timed out" in str(e).lower():
                print("dsort host transport: no answer before the exchange deadline", flush=True)
                t.poisoned = "a collective timed out at the exchange deadline"
                return DSORT_ETIMEOUT
            raise
        return 0

    def _allgather(user, send, recv, nbytes):
        if t.poisoned:
            return DSORT_ECOMM
        try:
            mine = torch.frombuffer(bytearray(ctypes.string_at(send, nbytes)), dtype=torch.uint8) \
                if nbytes else torch.empty(0, dtype=torch.uint8)
            outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
            if pg is None:
                work = dist.all_gather(outs, mine, async_op=True)
            else:
                work = pg.allgather([outs], [mine])
            rc = _wait(work)
            if rc:
                return rc
            if nbytes:
                whole = torch.cat(outs).numpy()
                ctypes.memmove(recv, whole.ctypes.data, whole.nbytes)
            return 0
        except Exception as e:  # pragma: no cover - reported through the C error path
            print("dsort host transport allgather:", e, flush=True)
            return 1

    def _alltoallv(user, send, sc, sd, recv, rc, rd):
        if t.poisoned:
            return DSORT_ECOMM
        try:
            scounts = [int(sc[i]) for i in range(world)]
            rcounts = [int(rc[i]) for i in range(world)]
            chunks = b"".join(ctypes.string_at(send + int(sd[i]), scounts[i]) if scounts[i] else b""
                              for i in range(world))
            inp = torch.frombuffer(bytearray(chunks), dtype=torch.uint8) if chunks else torch.empty(0, dtype=torch.uint8)
            out = torch.empty(sum(rcounts), dtype=torch.uint8)
            if pg is None:
                work = dist.all_to_all_single(out, inp, output_split_sizes=rcounts, input_split_sizes=scounts,
                                              async_op=True)
            else:
                work = pg.alltoall_base(out, inp, rcounts, scounts)
            r = _wait(work)
            if r:
                return r
            o = out.numpy()
            off = 0
            for i in range(world):
                if rcounts[i]:
                    ctypes.memmove(recv + int(rd[i]), o.ctypes.data + off, rcounts[i])
                off += rcounts[i]
            return 0
        except Exception as e:  # pragma: no cover
            print("dsort host transport alltoallv:", e, flush=True)
            return 1

    t = Transport(None, ALLGATHER_FN(_allgather), ALLTOALLV_FN(_alltoallv))
    t._keep = (_allgather, _alltoallv)  # the C side holds raw function pointers
    t.deadline_fn = deadline_fn
    t.poisoned = None  # (set by the first timeout: the group must be rebuilt)
    return t


_lib = None
P = ctypes.c_void_p
SZ = ctypes.c_size_t
U64 = ctypes.c_uint64
I32 = ctypes.c_int32


def load():
    """Load lib/libdsort.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DsortError(f"{LIB_PATH} missing: build it with `make -C {HERE}` (no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    sig = {
        "dsort_init": (ctypes.c_int, [ctypes.POINTER(P), ctypes.c_int]),
        "dsort_finalize": (ctypes.c_int, [P]),
        "dsort_last_error": (ctypes.c_char_p, [P]),
        "dsort_version": (ctypes.c_char_p, []),
        "dsort_get_stats": (ctypes.c_int, [P, ctypes.POINTER(Stats)]),
        "dsort_synchronize": (ctypes.c_int, [P]),
        "dsort_set_option": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int64]),
        "dsort_get_option": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
        "dsort_sort_stages": (ctypes.c_int, [P, SZ, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "dsort_sample_sort_stages": (ctypes.c_int, [P, SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.POINTER(ctypes.c_int)]),
        "dsort_sort_i32": (ctypes.c_int, [P, P, SZ]),
        "dsort_sort_i64": (ctypes.c_int, [P, P, SZ]),
        "dsort_sort_dev_i32": (ctypes.c_int, [P, P, SZ, P]),
        "dsort_sort_dev_i64": (ctypes.c_int, [P, P, SZ, P]),
        "dsort_sort_dev_copy_i32": (ctypes.c_int, [P, P, P, SZ, P]),
        "dsort_sort_dev_copy_i64": (ctypes.c_int, [P, P, P, SZ, P]),
        "dsort_merge_i32": (ctypes.c_int, [P, P, P, ctypes.c_int, P]),
        "dsort_merge_i64": (ctypes.c_int, [P, P, P, ctypes.c_int, P]),
        "dsort_merge_dev_i32": (ctypes.c_int, [P, P, P, ctypes.c_int, P, P]),
        "dsort_merge_dev_i64": (ctypes.c_int, [P, P, P, ctypes.c_int, P, P]),
        "dsort_comm_unique_id": (ctypes.c_int, [P]),
        "dsort_comm_init": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, P]),
        "dsort_comm_init_transport": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Transport)]),
        "dsort_comm_abort": (ctypes.c_int, [P]),
        "dsort_comm_deadline_ms": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_int64)]),
        "dsort_comm_destroy": (ctypes.c_int, [P]),
        "dsort_sample_sort_dev_i32": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(P), ctypes.POINTER(SZ), P]),
        "dsort_sample_sort_dev_i64": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(P), ctypes.POINTER(SZ), P]),
        "dsort_sample_merge_dev_i32": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(P), ctypes.POINTER(SZ), P]),
        "dsort_sample_merge_dev_i64": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(P), ctypes.POINTER(SZ), P]),
        "dsort_plan_splitters_i32": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, P, P, P, P, P]),
        "dsort_plan_splitters_i64": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, P, P, P, P, P]),
        "dsort_plan_cuts_i32": (ctypes.c_int, [P, SZ, ctypes.c_int, ctypes.c_int, P, P, P, P]),
        "dsort_plan_cuts_i64": (ctypes.c_int, [P, SZ, ctypes.c_int, ctypes.c_int, P, P, P, P]),
        "dsort_plan_sample_positions": (ctypes.c_int, [SZ, ctypes.c_int, P]),
        "dsort_gen_uniform_i32": (ctypes.c_int, [P, P, SZ, U64, U64, P]),
        "dsort_gen_uniform_i64": (ctypes.c_int, [P, P, SZ, U64, U64, P]),
        "dsort_gen_zipf_i64": (ctypes.c_int, [P, P, SZ, U64, U64, P]),
        "dsort_fingerprint_i32": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
        "dsort_fingerprint_i64": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
        "dsort_count_descents_i32": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(U64)]),
        "dsort_count_descents_i64": (ctypes.c_int, [P, P, SZ, ctypes.POINTER(U64)]),
        "dsort_dev_alloc": (ctypes.c_int, [P, ctypes.POINTER(P), SZ]),
        "dsort_dev_free": (ctypes.c_int, [P, P]),
        "dsort_copy_h2d": (ctypes.c_int, [P, P, P, SZ]),
        "dsort_copy_d2h": (ctypes.c_int, [P, P, P, SZ]),
        "dsort_copy_d2d": (ctypes.c_int, [P, P, P, SZ]),
        "dsort_host_register": (ctypes.c_int, [P, P, SZ]),
        "dsort_host_unregister": (ctypes.c_int, [P, P]),
        "dsort_write_text_i32": (ctypes.c_int, [ctypes.c_char_p, P, SZ]),
        "dsort_format_text_dev_i32": (ctypes.c_int, [P, P, SZ, P, SZ, ctypes.POINTER(SZ), P]),
        "dsort_parse_text_dev_i32": (ctypes.c_int, [P, P, SZ, P, SZ, ctypes.POINTER(SZ), P]),
        "dsort_parse_text_i32": (ctypes.c_int, [P, ctypes.c_char_p, SZ, P, SZ, ctypes.POINTER(SZ)]),
        "dsort_format_text_i32": (ctypes.c_int, [P, P, SZ, P, SZ, ctypes.POINTER(SZ)]),
        "dsort_argsort_dev_i32": (ctypes.c_int, [P, P, P, P, SZ, P]),
        "dsort_sort_pairs_dev_i32": (ctypes.c_int, [P, P, P, P, P, SZ, P]),
        "dsort_gather_dev": (ctypes.c_int, [P, P, P, P, SZ, ctypes.c_int, P]),
        "dsort_argsort_i32": (ctypes.c_int, [P, P, P, P, SZ]),
        "dsort_sample_argsort_dev_i32": (ctypes.c_int, [P, P, SZ, U64, ctypes.POINTER(P), ctypes.POINTER(P),
                                                        ctypes.POINTER(SZ), P]),
        "dsort_sample_sort_pairs_dev_i32": (ctypes.c_int, [P, P, P, SZ, ctypes.POINTER(P), ctypes.POINTER(P),
                                                           ctypes.POINTER(SZ), P]),
        "dsort_sample_gather_dev": (ctypes.c_int, [P, P, SZ, U64, P, SZ, P, ctypes.c_int, P]),
        "dsort_plan_gather_table": (ctypes.c_int, [ctypes.c_int, P, P, P, P, P, ctypes.POINTER(ctypes.c_int)]),
        "dsort_plan_gather_route": (ctypes.c_int, [ctypes.c_int, P, P, P, ctypes.c_int, P, SZ, P, P]),
        "dsort_argsort_dev_i64": (ctypes.c_int, [P, P, P, P, SZ, P]),
        "dsort_argsort_i64": (ctypes.c_int, [P, P, P, P, SZ]),
        "dsort_sort_records_dev_i64": (ctypes.c_int, [P, P, P, P, P, SZ, ctypes.c_int, P]),
        "dsort_plan_argsort_i64": (ctypes.c_int, [SZ, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int),
                                                  ctypes.POINTER(ctypes.c_int)]),
        "dsort_sample_argsort_dev_i64": (ctypes.c_int, [P, P, SZ, U64, ctypes.POINTER(P), ctypes.POINTER(P),
                                                        ctypes.POINTER(SZ), P]),
        "dsort_plan_sample_argsort_i64": (ctypes.c_int, [ctypes.c_int, P, P, P, P, ctypes.POINTER(ctypes.c_int),
                                                         ctypes.POINTER(ctypes.c_int)]),
        "dsort_key_encode": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, P, P, SZ]),
        "dsort_key_decode": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, P, P, SZ]),
        "dsort_sort_dev_keys": (ctypes.c_int, [P, P, SZ, ctypes.c_int, ctypes.c_int, P]),
        "dsort_sort_dev_copy_keys": (ctypes.c_int, [P, P, P, SZ, ctypes.c_int, ctypes.c_int, P]),
        "dsort_sort_keys": (ctypes.c_int, [P, P, SZ, ctypes.c_int, ctypes.c_int]),
        "dsort_argsort_dev_keys": (ctypes.c_int, [P, P, P, P, SZ, ctypes.c_int, ctypes.c_int, P]),
        "dsort_argsort_keys": (ctypes.c_int, [P, P, P, P, SZ, ctypes.c_int, ctypes.c_int]),
        "dsort_sort_pairs_dev_keys": (ctypes.c_int, [P, P, P, P, P, SZ, ctypes.c_int, ctypes.c_int, P]),
        "dsort_sort_records_dev_keys": (ctypes.c_int, [P, P, P, P, P, SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                       P]),
        "dsort_sample_sort_dev_keys": (ctypes.c_int, [P, P, SZ, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P),
                                                      ctypes.POINTER(SZ), P]),
        "dsort_sample_argsort_dev_keys": (ctypes.c_int, [P, P, SZ, U64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P),
                                                         ctypes.POINTER(P), ctypes.POINTER(SZ), P]),
        "dsort_plan_topk": (ctypes.c_int, [SZ, SZ, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_int)]),
        "dsort_topk_dev_keys": (ctypes.c_int, [P, P, SZ, SZ, ctypes.c_int, ctypes.c_int, P, P, P]),
        "dsort_topk_keys": (ctypes.c_int, [P, P, SZ, SZ, ctypes.c_int, ctypes.c_int, P, P]),
        "dsort_sample_topk_dev_keys": (ctypes.c_int, [P, P, SZ, U64, SZ, ctypes.c_int, ctypes.c_int, P, P, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def _sfx(dtype):
    dt = np.dtype(dtype)
    if dt == np.int32:
        return "i32"
    if dt == np.int64:
        return "i64"
    raise DsortError(f"unsupported key type {dt} (int32 / int64)")


def _key_name(dtype_name, itemsize, key_type):
    """The key type name ("f32", ...) of an array or tensor: its own dtype's, or the `key_type`
    override, whose width must be the element size (an int32 array sorted as "u32")."""
    if key_type is None:
        if dtype_name is None:
            raise DsortError("unsupported key dtype (float32/float64/uint32/uint64/int32/int64)")
        return dtype_name
    if key_type not in KEY_TYPES:
        raise DsortError(f"unknown key_type {key_type!r} (one of {', '.join(KEY_TYPES)})")
    if int(key_type[1:]) != 8 * itemsize:
        raise DsortError(f"key_type {key_type!r} does not match the {itemsize}-byte elements")
    return key_type


def _np_key(a, key_type):
    return _key_name(_KEY_OF_NP.get(a.dtype), a.dtype.itemsize, key_type)


def key_encode(keys, descending=False, key_type=None):
    """The order-preserving words of a numpy key array (dsort_key_encode, the rule the kernels run):
    a new signed-integer array of the keys' width whose signed order is the keys' order (float:
    IEEE totalOrder), reversed with descending=True."""
    keys = np.ascontiguousarray(keys)
    name = _np_key(keys, key_type)
    words = np.empty(keys.shape, np.int32 if keys.dtype.itemsize == 4 else np.int64)
    _check(None, load().dsort_key_encode(KEY_TYPES[name], ORDER_DESCENDING if descending else 0, _ptr(keys),
                                         _ptr(words), keys.size))
    return words


def key_decode(words, key_type, descending=False):
    """The keys of the words key_encode made (dsort_key_decode): a new array of the numpy type of
    `key_type` ("f32", "u64", ...), bit-exact."""
    words = np.ascontiguousarray(words)
    name = _key_name(None, words.dtype.itemsize, key_type)
    keys = np.empty(words.shape, _NP_OF_KEY[name])
    _check(None, load().dsort_key_decode(KEY_TYPES[name], ORDER_DESCENDING if descending else 0, _ptr(words),
                                         _ptr(keys), words.size))
    return keys


# ----------------------------------------------------------------- host-only planning helpers
def plan_sample_positions(n, s):
    lib = load()
    idx = np.zeros(s, np.uint64)
    _check(None, lib.dsort_plan_sample_positions(n, s, _ptr(idx)))
    return idx


def plan_splitters(samples, idx, nranks):
    """samples: (nranks*s,) keys, per-rank sorted blocks; returns (val, rank, index) arrays."""
    lib = load()
    samples = np.ascontiguousarray(samples)
    s = samples.size // nranks
    sv = np.zeros(max(nranks - 1, 1), samples.dtype)
    sr = np.zeros(max(nranks - 1, 1), np.int32)
    si = np.zeros(max(nranks - 1, 1), np.uint64)
    f = getattr(lib, f"dsort_plan_splitters_{_sfx(samples.dtype)}")
    _check(None, f(nranks, s, _ptr(samples), _ptr(np.ascontiguousarray(idx, np.uint64)),
                   _ptr(sv), _ptr(sr), _ptr(si)))
    return sv[:nranks - 1], sr[:nranks - 1], si[:nranks - 1]


def plan_cuts(sorted_keys, my_rank, nranks, sv, sr, si):
    lib = load()
    sorted_keys = np.ascontiguousarray(sorted_keys)
    cuts = np.zeros(nranks + 1, np.uint64)
    f = getattr(lib, f"dsort_plan_cuts_{_sfx(sorted_keys.dtype)}")
    sv = np.ascontiguousarray(sv, sorted_keys.dtype)
    sr = np.ascontiguousarray(sr, np.int32)
    si = np.ascontiguousarray(si, np.uint64)
    _check(None, f(_ptr(sorted_keys), sorted_keys.size, my_rank, nranks, _ptr(sv), _ptr(sr),
                   _ptr(si), _ptr(cuts)))
    return cuts


def plan_gather_table(first, count):
    """The distributed gather's owner table (dsort_plan_gather_table) from every rank's range
    [first[r], first[r] + count[r]): (lo, hi, owner) of the non-empty ranges, sorted by lo."""
    lib = load()
    first = np.ascontiguousarray(first, np.uint64)
    count = np.ascontiguousarray(count, np.uint64)
    nranks = first.size
    assert count.size == nranks
    lo, hi = np.zeros(nranks, np.uint64), np.zeros(nranks, np.uint64)
    owner = np.zeros(nranks, np.int32)
    nr = ctypes.c_int()
    _check(None, lib.dsort_plan_gather_table(nranks, _ptr(first), _ptr(count), _ptr(lo), _ptr(hi), _ptr(owner),
                                             ctypes.byref(nr)))
    return lo[:nr.value], hi[:nr.value], owner[:nr.value]


def plan_gather_route(lo, hi, owner, nranks, idx):
    """The gather's routing on the host (dsort_plan_gather_route): (counts, pos); counts has
    nranks + 1 entries, the last counting the indices nobody owns, pos[j] is index j's place in the
    owner-major, input-order-stable request layout."""
    lib = load()
    lo = np.ascontiguousarray(lo, np.uint64)
    hi = np.ascontiguousarray(hi, np.uint64)
    owner = np.ascontiguousarray(owner, np.int32)
    idx = np.ascontiguousarray(idx, np.uint32)
    counts = np.zeros(nranks + 1, np.uint64)
    pos = np.zeros(max(idx.size, 1), np.uint64)
    _check(None, lib.dsort_plan_gather_route(lo.size, _ptr(lo), _ptr(hi), _ptr(owner), nranks, _ptr(idx), idx.size,
                                             _ptr(counts), _ptr(pos)))
    return counts, pos[:idx.size]


def plan_argsort_i64(n, key_min, key_max):
    """The int64 argsort's host rule (dsort_plan_argsort_i64): (idx_bits, passes) for n keys whose
    smallest and largest are key_min and key_max."""
    b, p = ctypes.c_int(), ctypes.c_int()
    _check(None, load().dsort_plan_argsort_i64(n, key_min, key_max, ctypes.byref(b), ctypes.byref(p)))
    return b.value, p.value


def plan_sample_argsort_i64(first, count, key_min, key_max):
    """The host rule of the int64 argsort across ranks (dsort_plan_sample_argsort_i64):
    (idx_bits, passes) from every rank's range [first[r], first[r] + count[r]) and the smallest and
    largest key it holds (ignored where count[r] is 0)."""
    first = np.ascontiguousarray(first, np.uint64)
    count = np.ascontiguousarray(count, np.uint64)
    key_min = np.ascontiguousarray(key_min, np.int64)
    key_max = np.ascontiguousarray(key_max, np.int64)
    assert count.size == first.size == key_min.size == key_max.size
    b, p = ctypes.c_int(), ctypes.c_int()
    _check(None, load().dsort_plan_sample_argsort_i64(first.size, _ptr(first), _ptr(count), _ptr(key_min),
                                                      _ptr(key_max), ctypes.byref(b), ctypes.byref(p)))
    return b.value, p.value


def plan_topk(n, k, key_bytes, path=-1):
    """The top-k host rule (dsort_plan_topk): (path, digits) for the k first of n keys of key_bytes
    bytes -- path 0 nothing to do, 1 the select path, 2 the full argsort and its first k; `path`
    is the value of the "topk_path" option (-1: the rule, 0 / 1: forced); digits = the histogram passes
    of the select path for the width."""
    p, d = ctypes.c_int(), ctypes.c_int()
    _check(None, load().dsort_plan_topk(n, k, key_bytes, path, ctypes.byref(p), ctypes.byref(d)))
    return p.value, d.value


def write_text_i32(path, keys):
    lib = load()
    keys = np.ascontiguousarray(keys, np.int32)
    _check(None, lib.dsort_write_text_i32(os.fsencode(path), _ptr(keys), keys.size))


def _check(ctx, rc):
    if rc != DSORT_OK:
        msg = load().dsort_last_error(ctx).decode() if ctx else ""
        err = DsortError(f"libdsort error {rc} ({ERRORS.get(rc, '?')}): {msg}")
        err.rc = rc
        raise err
    return rc


class Context:
    """One libdsort context bound to one GPU (dsort_init / dsort_finalize)."""

    def __init__(self, device=0):
        self.lib = load()
        h = P()
        rc = self.lib.dsort_init(ctypes.byref(h), device)
        if rc != DSORT_OK:
            raise DsortError(f"dsort_init(device={device}) failed: {rc} ({ERRORS.get(rc, '?')}); "
                             "a gfx950 GPU is required (no CPU fallback)")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.dsort_finalize(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        return _check(self.h, rc)

    # ---------------- options (dsort_set_option) -----------------------------------------
    @staticmethod
    def _opt(name):
        return OPTIONS[name]  # (ABI 6 dropped ABI 2's "kill_after_pass" alias)

    def set_option(self, name, value):
        self.check(self.lib.dsort_set_option(self.h, self._opt(name), int(value)))

    def get_option(self, name):
        v = ctypes.c_int64()
        self.check(self.lib.dsort_get_option(self.h, self._opt(name), ctypes.byref(v)))
        return v.value

    # Not part of the ABI (debug entries of csrc/dsort_wave.hip, outside include/dsort.h): the second
    # level's arithmetic sub-bucket map.
    def sub_arith_mode(self, mode):
        """-1 = per bucket by the sample rule (default), 0 = off, 2 = every bucket whose span allows it (tests)."""
        f = self.lib.dsort_debug_sub_arith_mode
        f.restype, f.argtypes = ctypes.c_int, [P, ctypes.c_int]
        self.check(f(self.h, int(mode)))

    def sub_arith_counts(self):
        """(buckets of several sub-buckets, those on the arithmetic map) of the last bucketed sort."""
        out = (ctypes.c_uint32 * 2)()
        f = self.lib.dsort_debug_sub_arith
        f.restype, f.argtypes = ctypes.c_int, [P, P]
        self.check(f(self.h, ctypes.cast(out, P)))
        return int(out[0]), int(out[1])

    # Likewise the first level's arithmetic bucket map (csrc/dsort_bucket.h, BkMap.ar).
    def bucket_arith_mode(self, mode):
        """-1 = by the sample rule (default), 0 = off, 2 = whenever the samples' key range allows it (tests)."""
        f = self.lib.dsort_debug_bucket_arith_mode
        f.restype, f.argtypes = ctypes.c_int, [P, ctypes.c_int]
        self.check(f(self.h, int(mode)))

    def bucket_arith(self):
        """True if the first level of the last bucketed sort ran on the arithmetic bucket map."""
        out = (ctypes.c_uint32 * 1)()
        f = self.lib.dsort_debug_bucket_arith
        f.restype, f.argtypes = ctypes.c_int, [P, P]
        self.check(f(self.h, ctypes.cast(out, P)))
        return bool(out[0])

    @contextlib.contextmanager
    def options(self, **kw):
        """Sets options for the body of a with-statement and restores the previous values."""
        old = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

    def sort_stages(self, n, key_bytes=4):
        """Kill points of a sort of n keys under this context's options (dsort_sort_stages)."""
        m = ctypes.c_int()
        self.check(self.lib.dsort_sort_stages(self.h, n, key_bytes, ctypes.byref(m)))
        return m.value

    # ---------------- host-buffer entry points (reference drop-ins) ----------------------
    def sort(self, keys, descending=False, key_type=None):
        """In-place sort of a host numpy array (dsort_sort_i32 / _i64; any other key type, a
        `key_type` override or descending=True: dsort_sort_keys)."""
        assert keys.flags.c_contiguous
        name = _np_key(keys, key_type)
        if name in ("i32", "i64") and not descending:
            f = getattr(self.lib, f"dsort_sort_{name}")
            self.check(f(self.h, _ptr(keys), keys.size))
        else:
            self.check(self.lib.dsort_sort_keys(self.h, _ptr(keys), keys.size, KEY_TYPES[name],
                                                ORDER_DESCENDING if descending else 0))
        return keys

    def merge(self, runs):
        """Merge sorted host runs (dsort_merge_*); returns a new array."""
        runs = [np.ascontiguousarray(r) for r in runs]
        dt = runs[0].dtype if runs else np.dtype(np.int32)
        k = len(runs)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[r.ctypes.data for r in runs])
        lens = (ctypes.c_size_t * max(k, 1))(*[r.size for r in runs])
        out = np.empty(sum(r.size for r in runs), dt)
        f = getattr(self.lib, f"dsort_merge_{_sfx(dt)}")
        self.check(f(self.h, ctypes.cast(ptrs, P), ctypes.cast(lens, P), k, _ptr(out)))
        return out

    # ---------------- device entry points (torch tensors) --------------------------------
    @staticmethod
    def _stream():
        # torch's default stream is HIP's null stream (handle 0); NULL would select the
        # context's own non-blocking stream, which is not ordered with torch's work.
        h = torch.cuda.current_stream().cuda_stream
        return ctypes.c_void_p(h if h else 1)  # 1 == DSORT_NULL_STREAM

    @staticmethod
    def _tsfx(t):
        if t.dtype == torch.int32:
            return "i32"
        if t.dtype == torch.int64:
            return "i64"
        raise DsortError(f"unsupported tensor dtype {t.dtype}")

    @staticmethod
    def _tkey(t, key_type=None, descending=False):
        """(name, typed) of a key tensor: its key type name and whether the call goes to the *_keys
        entry points (anything but signed integers ascending)."""
        names = {torch.int32: "i32", torch.float32: "f32", torch.int64: "i64", torch.float64: "f64"}
        for dt, nm in (("uint32", "u32"), ("uint64", "u64")):
            if hasattr(torch, dt):
                names[getattr(torch, dt)] = nm
        name = _key_name(names.get(t.dtype), t.element_size(), key_type)
        return name, bool(descending) or name not in ("i32", "i64")

    @staticmethod
    def _keys1d(t, what, n=None, like=None):
        if not t.is_contiguous() or t.dim() != 1 or (like is not None and t.dtype != like.dtype):
            raise DsortError(f"{what}: a contiguous 1-d tensor of the keys' dtype is required")
        if n is not None and t.numel() != n:
            raise DsortError(f"{what}: {t.numel()} elements, expected {n}")
        return t

    def sort_dev(self, t, out=None, descending=False, key_type=None):
        """Sort a CUDA tensor in place, or into `out` (dsort_sort_dev[_copy]_i32 / _i64; float and
        unsigned dtypes, a `key_type` override such as "u32" on an int32 tensor, or descending=True:
        dsort_sort_dev[_copy]_keys).  Floats sort in IEEE totalOrder (dsort.h)."""
        name, typed = self._tkey(t, key_type, descending)
        if typed:
            kt, fl = KEY_TYPES[name], ORDER_DESCENDING if descending else 0
            if out is None:
                self.check(self.lib.dsort_sort_dev_keys(self.h, t.data_ptr(), t.numel(), kt, fl, self._stream()))
                return t
            assert out.numel() == t.numel() and out.dtype == t.dtype
            self.check(self.lib.dsort_sort_dev_copy_keys(self.h, t.data_ptr(), out.data_ptr(), t.numel(), kt, fl,
                                                         self._stream()))
            return out
        sfx = name
        if out is None:
            self.check(getattr(self.lib, f"dsort_sort_dev_{sfx}")(self.h, t.data_ptr(), t.numel(),
                                                                   self._stream()))
            return t
        assert out.numel() == t.numel() and out.dtype == t.dtype
        self.check(getattr(self.lib, f"dsort_sort_dev_copy_{sfx}")(self.h, t.data_ptr(), out.data_ptr(),
                                                                    t.numel(), self._stream()))
        return out

    def merge_dev(self, t, lens, out):
        sfx = self._tsfx(t)
        k = len(lens)
        la = (ctypes.c_size_t * max(k, 1))(*[int(x) for x in lens])
        self.check(getattr(self.lib, f"dsort_merge_dev_{sfx}")(self.h, t.data_ptr(), ctypes.cast(la, P), k,
                                                                out.data_ptr(), self._stream()))
        return out

    # ---------------- argsort, key-value sort, gather (dsort.h, ABI 7; int64 keys: ABI 10) ----
    @staticmethod
    def _i32(t, what, n=None, dtype=None):
        dtype = torch.int32 if dtype is None else dtype
        if t.dtype != dtype or not t.is_contiguous() or t.dim() != 1:
            raise DsortError(f"{what}: a contiguous 1-d {str(dtype).split('.')[-1]} tensor is required")
        if n is not None and t.numel() != n:
            raise DsortError(f"{what}: {t.numel()} elements, expected {n}")
        return t

    def argsort_dev(self, keys, idx_out=None, keys_out=None, descending=False, key_type=None):
        """Stable argsort of an int32 or int64 CUDA tensor (dsort_argsort_dev_i32 / _i64): returns
        (keys_out, idx).  idx[j] is the position in `keys` of the j-th smallest key, equal keys
        in input order.  idx is an int32 tensor holding the uint32 bit pattern (torch has no
        uint32 arithmetic): non-negative, and usable as an index, for n < 2^31.  keys_out=None:
        the sorted keys are not produced (None is returned for them); keys_out may be `keys`.
        Float and unsigned keys, a `key_type` override or descending=True go to
        dsort_argsort_dev_keys: the order of dsort.h's "Key types and order", equal keys in ascending
        input position in either direction."""
        name, typed = self._tkey(keys, key_type, descending)
        if typed:
            n = self._keys1d(keys, "keys").numel()
            if idx_out is None:
                idx_out = torch.empty(n, dtype=torch.int32, device=keys.device)
            self._i32(idx_out, "idx_out", n)
            ko = None if keys_out is None else self._keys1d(keys_out, "keys_out", n, keys).data_ptr()
            self.check(self.lib.dsort_argsort_dev_keys(self.h, keys.data_ptr(), ko, idx_out.data_ptr(), n,
                                                       KEY_TYPES[name], ORDER_DESCENDING if descending else 0,
                                                       self._stream()))
            return keys_out, idx_out
        kt = torch.int64 if keys.dtype == torch.int64 else torch.int32
        n = self._i32(keys, "keys", dtype=kt).numel()
        if idx_out is None:
            idx_out = torch.empty(n, dtype=torch.int32, device=keys.device)
        self._i32(idx_out, "idx_out", n)
        ko = None if keys_out is None else self._i32(keys_out, "keys_out", n, kt).data_ptr()
        f = self.lib.dsort_argsort_dev_i64 if kt == torch.int64 else self.lib.dsort_argsort_dev_i32
        self.check(f(self.h, keys.data_ptr(), ko, idx_out.data_ptr(), n, self._stream()))
        return keys_out, idx_out

    def sort_records_dev(self, keys, records, keys_out=None, out=None, descending=False, key_type=None):
        """Stable sort of records by an int64 key (dsort_sort_records_dev_i64): records[i] belongs
        to keys[i]; a record is one row of `records`, of 4, 8 or 16 bytes as for gather_dev; rows of
        equal keys keep their input order.  keys_out (None: not wanted; may be `keys`) gets the
        sorted keys.  Returns (keys_out, out), out holding the rows in key order.  Float and unsigned
        keys, a `key_type` override (key_type="i32": the record sort of int32 keys) or
        descending=True: dsort_sort_records_dev_keys."""
        name, typed = self._tkey(keys, key_type, descending)
        typed = typed or key_type is not None
        n = self._keys1d(keys, "keys").numel() if typed else self._i32(keys, "keys", dtype=torch.int64).numel()
        if not records.is_contiguous() or records.dim() < 1 or int(records.shape[0]) != n:
            raise DsortError("sort_records_dev: one contiguous record per key is required")
        rec = records.element_size()
        for d in records.shape[1:]:
            rec *= int(d)
        if rec not in (4, 8, 16):
            raise DsortError(f"sort_records_dev: records of {rec} bytes (4, 8 or 16)")
        if out is None:
            out = torch.empty_like(records)
        if out.dtype != records.dtype or out.shape != records.shape or not out.is_contiguous():
            raise DsortError("sort_records_dev: out must match the records' type and shape")
        if typed:
            ko = None if keys_out is None else self._keys1d(keys_out, "keys_out", n, keys).data_ptr()
            self.check(self.lib.dsort_sort_records_dev_keys(self.h, keys.data_ptr(), ko, records.data_ptr(),
                                                            out.data_ptr(), n, rec, KEY_TYPES[name],
                                                            ORDER_DESCENDING if descending else 0, self._stream()))
            return keys_out, out
        ko = None if keys_out is None else self._i32(keys_out, "keys_out", n, torch.int64).data_ptr()
        self.check(self.lib.dsort_sort_records_dev_i64(self.h, keys.data_ptr(), ko, records.data_ptr(),
                                                       out.data_ptr(), n, rec, self._stream()))
        return keys_out, out

    def sort_pairs_dev(self, keys, vals, keys_out=None, vals_out=None, descending=False, key_type=None):
        """Key-value sort of int32 CUDA tensors (dsort_sort_pairs_dev_i32): ascending by key, equal
        keys by value as UNSIGNED 32-bit.  In place when the outputs are None.  Returns
        (keys_out, vals_out).  float32 / uint32 keys, a `key_type` override or descending=True:
        dsort_sort_pairs_dev_keys (4-byte key types only; equal keys still by value ascending)."""
        name, typed = self._tkey(keys, key_type, descending)
        if typed:
            n = self._keys1d(keys, "keys").numel()
            self._i32(vals, "vals", n)
            keys_out = keys if keys_out is None else self._keys1d(keys_out, "keys_out", n, keys)
            vals_out = vals if vals_out is None else self._i32(vals_out, "vals_out", n)
            self.check(self.lib.dsort_sort_pairs_dev_keys(self.h, keys.data_ptr(), vals.data_ptr(), keys_out.data_ptr(),
                                                          vals_out.data_ptr(), n, KEY_TYPES[name],
                                                          ORDER_DESCENDING if descending else 0, self._stream()))
            return keys_out, vals_out
        n = self._i32(keys, "keys").numel()
        self._i32(vals, "vals", n)
        keys_out = keys if keys_out is None else self._i32(keys_out, "keys_out", n)
        vals_out = vals if vals_out is None else self._i32(vals_out, "vals_out", n)
        self.check(self.lib.dsort_sort_pairs_dev_i32(self.h, keys.data_ptr(), vals.data_ptr(), keys_out.data_ptr(),
                                                     vals_out.data_ptr(), n, self._stream()))
        return keys_out, vals_out

    def gather_dev(self, src, idx, out):
        """out[i] = src[idx[i]] along dim 0 (dsort_gather_dev).  A record is one row of `src`:
        element_size * the trailing dimensions, which must be 4, 8 or 16 bytes.  idx: int32 (the
        argsort's uint32 bit pattern)."""
        n = self._i32(idx, "idx").numel()
        if not src.is_contiguous() or not out.is_contiguous() or src.dim() < 1:
            raise DsortError("gather: contiguous tensors are required")
        rec = src.element_size()
        for d in src.shape[1:]:
            rec *= int(d)
        if rec not in (4, 8, 16):
            raise DsortError(f"gather: records of {rec} bytes (4, 8 or 16)")
        if out.dtype != src.dtype or tuple(out.shape) != (n,) + tuple(src.shape[1:]):
            raise DsortError("gather: out must hold len(idx) records of src's type and row shape")
        self.check(self.lib.dsort_gather_dev(self.h, src.data_ptr(), idx.data_ptr(), out.data_ptr(), n, rec,
                                             self._stream()))
        return out

    def argsort(self, keys, descending=False, key_type=None):
        """Host form (dsort_argsort_i32 / _i64): stable argsort of a numpy array -- int64 as it is,
        anything else as int32; returns (sorted_keys, idx) as new arrays, idx of dtype uint32.
        float32 / float64 / uint32 / uint64 arrays, a `key_type` override or descending=True:
        dsort_argsort_keys on the array as it is."""
        typed = descending or key_type is not None or (
            isinstance(keys, np.ndarray) and _KEY_OF_NP.get(keys.dtype) in ("u32", "f32", "u64", "f64"))
        if typed:
            keys = np.ascontiguousarray(keys)
            name = _np_key(keys, key_type)
            out = np.empty_like(keys)
            idx = np.empty(keys.size, np.uint32)
            self.check(self.lib.dsort_argsort_keys(self.h, _ptr(keys), _ptr(out), _ptr(idx), keys.size,
                                                   KEY_TYPES[name], ORDER_DESCENDING if descending else 0))
            return out, idx
        wide = isinstance(keys, np.ndarray) and keys.dtype == np.int64
        keys = np.ascontiguousarray(keys, np.int64 if wide else np.int32)
        out = np.empty_like(keys)
        idx = np.empty(keys.size, np.uint32)
        f = self.lib.dsort_argsort_i64 if wide else self.lib.dsort_argsort_i32
        self.check(f(self.h, _ptr(keys), _ptr(out), _ptr(idx), keys.size))
        return out, idx

    # ---------------- top-k selection (dsort.h, "top-k") ------------------------------------
    def _topk_outs(self, keys, k, keys_out, idx_out):
        if idx_out is None:
            idx_out = torch.empty(k, dtype=torch.int32, device=keys.device)
        self._i32(idx_out, "idx_out", k)
        if keys_out is None:
            keys_out = torch.empty(k, dtype=keys.dtype, device=keys.device)
        elif keys_out is False:  # not wanted: the C call gets NULL
            keys_out = None
        else:
            self._keys1d(keys_out, "keys_out", k, keys)
        return keys_out, idx_out

    def topk_dev(self, keys, k, descending=False, key_type=None, keys_out=None, idx_out=None):
        """The first k entries of argsort_dev(keys, descending=..., key_type=...) without the full
        sort (dsort_topk_dev_keys): returns (keys, idx), both sorted, idx an int32 tensor of uint32
        bit patterns as argsort_dev documents; descending=True gives the k largest.  Equal keys
        come in ascending position, and the lowest positions win where the cut falls inside a run
        of equal keys.  keys_out: a tensor of k elements of the keys' dtype, None (a new one) or
        False (the keys are not produced and None is returned for them); idx_out: a tensor of k
        int32, or None for a new one.  The "topk_path" option forces a path."""
        name, _ = self._tkey(keys, key_type, descending)
        n = self._keys1d(keys, "keys").numel()
        if k < 0 or k > n:
            raise DsortError(f"topk_dev: k = {k} outside 0..{n}")
        keys_out, idx_out = self._topk_outs(keys, k, keys_out, idx_out)
        self.check(self.lib.dsort_topk_dev_keys(self.h, keys.data_ptr() if n else None, n, k, KEY_TYPES[name],
                                                ORDER_DESCENDING if descending else 0,
                                                keys_out.data_ptr() if keys_out is not None and k else None,
                                                idx_out.data_ptr() if k else None, self._stream()))
        return keys_out, idx_out

    def topk(self, host_keys, k, descending=False, key_type=None):
        """Host form (dsort_topk_keys): the k first of the stable argsort of a numpy array in the
        typed order; returns (keys, idx) as new arrays, idx of dtype uint32."""
        keys = np.ascontiguousarray(host_keys)
        name = _np_key(keys, key_type)
        if k < 0 or k > keys.size:
            raise DsortError(f"topk: k = {k} outside 0..{keys.size}")
        out = np.empty(k, keys.dtype)
        idx = np.empty(k, np.uint32)
        self.check(self.lib.dsort_topk_keys(self.h, _ptr(keys), keys.size, k, KEY_TYPES[name],
                                            ORDER_DESCENDING if descending else 0, _ptr(out), _ptr(idx)))
        return out, idx

    def sample_topk_dev(self, keys, first, k, descending=False, key_type=None, keys_out=None, idx_out=None):
        """The global top-k over the communicator (dsort_sample_topk_dev_keys; collective): `keys`
        is this rank's chunk, holding the global positions first .. first + len(keys) - 1.  Every
        rank gets the same (keys, idx) of k elements, idx holding GLOBAL positions as uint32 bit
        patterns; the arguments as for topk_dev."""
        name, _ = self._tkey(keys, key_type, descending)
        n = self._keys1d(keys, "keys").numel()
        keys_out, idx_out = self._topk_outs(keys, k, keys_out, idx_out)
        self.check(self.lib.dsort_sample_topk_dev_keys(self.h, keys.data_ptr() if n else None, n, int(first), k,
                                                       KEY_TYPES[name], ORDER_DESCENDING if descending else 0,
                                                       keys_out.data_ptr() if keys_out is not None and k else None,
                                                       idx_out.data_ptr() if k else None, self._stream()))
        return keys_out, idx_out

    def gen_uniform(self, t, seed, first=0):
        sfx = self._tsfx(t)
        self.check(getattr(self.lib, f"dsort_gen_uniform_{sfx}")(self.h, t.data_ptr(), t.numel(), seed, first,
                                                                  self._stream()))
        return t

    def gen_zipf_i64(self, t, seed, first=0):
        assert t.dtype == torch.int64
        self.check(self.lib.dsort_gen_zipf_i64(self.h, t.data_ptr(), t.numel(), seed, first, self._stream()))
        return t

    def fingerprint(self, t, n=None):
        torch.cuda.current_stream().synchronize()
        s, x = U64(), U64()
        n = t.numel() if n is None else n
        self.check(getattr(self.lib, f"dsort_fingerprint_{self._tsfx(t)}")(self.h, t.data_ptr(), n,
                                                                            ctypes.byref(s), ctypes.byref(x)))
        return s.value, x.value

    def descents(self, t, n=None):
        torch.cuda.current_stream().synchronize()
        c = U64()
        n = t.numel() if n is None else n
        self.check(getattr(self.lib, f"dsort_count_descents_{self._tsfx(t)}")(self.h, t.data_ptr(), n,
                                                                               ctypes.byref(c)))
        return c.value

    def format_text(self, keys, text):
        """output.txt bytes of int32 CUDA tensor `keys` into uint8 CUDA tensor `text` (>= 12 bytes
        per key); returns the byte count (dsort_format_text_dev_i32)."""
        assert keys.dtype == torch.int32 and text.dtype == torch.uint8
        ln = ctypes.c_size_t()
        self.check(self.lib.dsort_format_text_dev_i32(self.h, keys.data_ptr(), keys.numel(), text.data_ptr(),
                                                      text.numel(), ctypes.byref(ln), self._stream()))
        return ln.value

    def parse_text(self, text, nbytes, keys):
        """Parse the first `nbytes` of uint8 CUDA tensor `text` (16-byte aligned) into int32 CUDA
        tensor `keys`; returns the token count (dsort_parse_text_dev_i32)."""
        assert keys.dtype == torch.int32 and text.dtype == torch.uint8 and nbytes <= text.numel()
        cnt = ctypes.c_size_t()
        self.check(self.lib.dsort_parse_text_dev_i32(self.h, text.data_ptr(), nbytes, keys.data_ptr(),
                                                     keys.numel(), ctypes.byref(cnt), self._stream()))
        return cnt.value

    def parse_text_host(self, raw):
        """Host bytes -> np.int32 keys through the GPU parser (dsort_parse_text_i32)."""
        cap = len(raw) // 2 + 1
        out = np.empty(cap, np.int32)
        cnt = ctypes.c_size_t()
        self.check(self.lib.dsort_parse_text_i32(self.h, raw, len(raw), _ptr(out), cap, ctypes.byref(cnt)))
        return out[:cnt.value]

    def format_text_host(self, keys):
        """np.int32 keys -> output.txt bytes through the GPU formatter (dsort_format_text_i32)."""
        keys = np.ascontiguousarray(keys, np.int32)
        buf = ctypes.create_string_buffer(12 * keys.size + 1)
        ln = ctypes.c_size_t()
        self.check(self.lib.dsort_format_text_i32(self.h, _ptr(keys), keys.size, buf, len(buf),
                                                  ctypes.byref(ln)))
        return buf.raw[:ln.value]

    def stats(self):
        st = Stats()
        self.check(self.lib.dsort_get_stats(self.h, ctypes.byref(st)))
        return st.as_dict()

    def synchronize(self):
        self.check(self.lib.dsort_synchronize(self.h))

    # ---------------- multi-GPU -----------------------------------------------------------
    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _check(None, load().dsort_comm_unique_id(buf))
        return bytes(buf.raw)

    def comm_init(self, nranks, rank, uid):
        assert len(uid) == 128
        buf = ctypes.create_string_buffer(uid, 128)
        self.check(self.lib.dsort_comm_init(self.h, nranks, rank, buf))

    def comm_init_transport(self, nranks, rank, transport):
        self._transport = transport  # keep the callbacks alive while the library may call them
        if getattr(transport, "deadline_fn", None) is None:
            transport.deadline_fn = self.deadline_ms  # the callbacks' waits end at the exchange deadline
        self.check(self.lib.dsort_comm_init_transport(self.h, nranks, rank, ctypes.byref(transport)))

    def deadline_ms(self):
        """Milliseconds left before the running sample sort's exchange deadline, -1 for none
        (dsort_comm_deadline_ms; for transport callbacks on the sorting thread)."""
        v = ctypes.c_int64()
        self.check(self.lib.dsort_comm_deadline_ms(self.h, ctypes.byref(v)))
        return v.value

    def comm_destroy(self):
        self.check(self.lib.dsort_comm_destroy(self.h))

    def comm_abort(self):
        self.check(self.lib.dsort_comm_abort(self.h))

    def sample_sort_dev(self, t, descending=False, key_type=None):
        """Returns (device pointer int, n_out) of this rank's slice (context-owned).  Float and
        unsigned keys, a `key_type` override or descending=True: dsort_sample_sort_dev_keys, the
        slice holding keys of the input's type."""
        name, typed = self._tkey(t, key_type, descending)
        outp, nout = P(), SZ()
        if typed:
            self.check(self.lib.dsort_sample_sort_dev_keys(self.h, t.data_ptr() if t.numel() else None, t.numel(),
                                                           KEY_TYPES[name], ORDER_DESCENDING if descending else 0,
                                                           ctypes.byref(outp), ctypes.byref(nout), self._stream()))
            return outp.value or 0, nout.value
        sfx = name
        self.check(getattr(self.lib, f"dsort_sample_sort_dev_{sfx}")(self.h, t.data_ptr(), t.numel(),
                                                                      ctypes.byref(outp), ctypes.byref(nout),
                                                                      self._stream()))
        return outp.value or 0, nout.value

    def sample_merge_dev(self, t):
        """Exchange half of the sample sort for an already sorted local run `t`
        (dsort_sample_merge_dev_*).  Returns (device pointer int, n_out) like sample_sort_dev."""
        sfx = self._tsfx(t)
        outp, nout = P(), SZ()
        self.check(getattr(self.lib, f"dsort_sample_merge_dev_{sfx}")(self.h, t.data_ptr(), t.numel(),
                                                                       ctypes.byref(outp), ctypes.byref(nout),
                                                                       self._stream()))
        return outp.value or 0, nout.value

    # ---------------- argsort and key-value sort across ranks (int32 keys; dsort.h, ABI 8) ----
    def _slices(self, ptrs, n, device, dtypes=None):
        """Fresh tensors (int32, or `dtypes`) holding the context-owned slices at `ptrs` (n elements
        each).  The unpack that fills them was queued on torch's current stream and dsort_copy_d2d
        runs on the context's: the stream is drained first."""
        torch.cuda.current_stream().synchronize()
        outs = []
        for p, dt in zip(ptrs, dtypes or [torch.int32] * len(ptrs)):
            t = torch.empty(n, dtype=dt, device=device)
            if n:
                self.check(self.lib.dsort_copy_d2d(self.h, t.data_ptr(), p.value, t.element_size() * n))
            outs.append(t)
        return outs

    def sample_argsort_dev(self, keys, first, descending=False, key_type=None):
        """Global stable argsort over the communicator (dsort_sample_argsort_dev_i32 / _i64): `keys`
        is this rank's chunk, int32 or int64, holding the global positions first .. first +
        len(keys) - 1.  Returns (sorted_keys, idx), this rank's slice of the global order as fresh
        CUDA tensors: the keys of the input's type, idx int32 holding global positions as uint32 bit
        patterns, as argsort_dev documents.  DSORT_ESTAGE of the int64 call leaves valid outputs: the
        DsortError then carries them as `.slices`.  Float and unsigned keys, a `key_type` override or
        descending=True: dsort_sample_argsort_dev_keys, equal keys in ascending global position."""
        name, typed = self._tkey(keys, key_type, descending)
        kp, ip, nout = P(), P(), SZ()
        if typed:
            kt = keys.dtype
            n = self._keys1d(keys, "keys").numel()
            rc = self.lib.dsort_sample_argsort_dev_keys(self.h, keys.data_ptr() if n else None, n, int(first),
                                                        KEY_TYPES[name], ORDER_DESCENDING if descending else 0,
                                                        ctypes.byref(kp), ctypes.byref(ip), ctypes.byref(nout),
                                                        self._stream())
        else:
            kt = torch.int64 if keys.dtype == torch.int64 else torch.int32
            n = self._i32(keys, "keys", dtype=kt).numel()
            f = self.lib.dsort_sample_argsort_dev_i64 if kt == torch.int64 else self.lib.dsort_sample_argsort_dev_i32
            rc = f(self.h, keys.data_ptr() if n else None, n, int(first), ctypes.byref(kp), ctypes.byref(ip),
                   ctypes.byref(nout), self._stream())
        try:
            self.check(rc)
        except DsortError as e:
            if e.rc == -7 and keys.element_size() == 8:  # DSORT_ESTAGE: every leg has run
                e.slices = tuple(self._slices((kp, ip), nout.value, keys.device, (kt, torch.int32)))
            raise
        k, i = self._slices((kp, ip), nout.value, keys.device, (kt, torch.int32))
        return k, i

    def sample_sort_pairs_dev(self, keys, vals):
        """Global key-value sort over the communicator (dsort_sample_sort_pairs_dev_i32): ascending
        by key, equal keys by value as UNSIGNED 32-bit.  Returns (sorted_keys, sorted_vals), this
        rank's slice as fresh int32 CUDA tensors (the values as uint32 bit patterns)."""
        n = self._i32(keys, "keys").numel()
        self._i32(vals, "vals", n)
        kp, vp, nout = P(), P(), SZ()
        self.check(self.lib.dsort_sample_sort_pairs_dev_i32(self.h, keys.data_ptr() if n else None,
                                                            vals.data_ptr() if n else None, n, ctypes.byref(kp),
                                                            ctypes.byref(vp), ctypes.byref(nout), self._stream()))
        k, v = self._slices((kp, vp), nout.value, keys.device)
        return k, v

    # ---------------- distributed record gather (dsort.h, ABI 9) ----------------------------
    def sample_gather_dev(self, records, first, idx, out=None):
        """out[j] = the record at GLOBAL position idx[j], wherever it lives
        (dsort_sample_gather_dev; collective).  `records` is this rank's contiguous CUDA tensor of
        records -- a record is one row, of 4, 8 or 16 bytes, as for gather_dev -- holding the global
        positions first .. first + len(records) - 1; idx is an int32 tensor of uint32 bit patterns,
        e.g. the index slice of sample_argsort_dev.  Returns `out`, shaped
        (len(idx),) + records.shape[1:]."""
        n = self._i32(idx, "idx").numel()
        if not records.is_contiguous() or records.dim() < 1:
            raise DsortError("gather: a contiguous tensor of records is required")
        rec = records.element_size()
        for d in records.shape[1:]:
            rec *= int(d)
        if rec not in (4, 8, 16):
            raise DsortError(f"gather: records of {rec} bytes (4, 8 or 16)")
        shape = (n,) + tuple(records.shape[1:])
        if out is None:
            out = torch.empty(shape, dtype=records.dtype, device=records.device)
        if out.dtype != records.dtype or tuple(out.shape) != shape or not out.is_contiguous():
            raise DsortError("gather: out must hold len(idx) records of the records' type and row shape")
        n_src = int(records.shape[0])
        self.check(self.lib.dsort_sample_gather_dev(self.h, records.data_ptr() if n_src else None, n_src, int(first),
                                                    idx.data_ptr() if n else None, n, out.data_ptr() if n else None,
                                                    rec, self._stream()))
        return out

    def sample_sort_records_dev(self, keys, records, first):
        """Distributed sort of records by an int32 or int64 key: sample_argsort_dev, then sample_gather_dev
        with the returned indices.  keys[i] is the key of records[i], global position first + i.
        Returns (sorted_keys, records_of_my_slice)."""
        if int(records.shape[0]) != keys.numel():
            raise DsortError("sample_sort_records_dev: one record per key is required")
        k, i = self.sample_argsort_dev(keys, first)
        return k, self.sample_gather_dev(records, first, i)

    def copy_d2h(self, host, dptr, nbytes):
        self.check(self.lib.dsort_copy_d2h(self.h, _ptr(host), dptr, nbytes))
        return host
