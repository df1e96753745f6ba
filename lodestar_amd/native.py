"""ctypes binding of libblsgpu.so (include/blsgpu.h).

This is the Python side of the drop-in boundary; the N-API addon described in
INTEGRATION.md binds the same symbols for Node.  There is no CPU fallback:
loading fails loudly when the HIP library is missing or no device is present.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import List, Optional, Sequence

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLSGPU_LIB", os.path.join(HERE, "libblsgpu.so"))

# status codes (include/blsgpu.h)
BGV_OK = 0
BLST_BAD_ENCODING = 1
BLST_POINT_NOT_ON_CURVE = 2
BLST_POINT_NOT_IN_GROUP = 3
BLST_PK_IS_INFINITY = 6
BLST_INVALID_SIZE = 8
BGV_E_EMPTY_AGGREGATE = 20
BGV_E_EMPTY_SET = 21
BGV_E_BAD_INDEX = 22
BGV_E_ARG = 23
BGV_E_DEVICE = 30
BGV_E_CLOSED = 32

MODE_WORKER = 0
MODE_PER_JOB = 1
PATH_BULK = 1
PATH_LATENCY = 2
PK_COMPRESSED = 48
PK_UNCOMPRESSED = 96
MAX_COMMITTEES = 16384
NO_COMMITTEE = 0xFFFFFFFF
NO_PROPOSER = 0xFFFFFFFF
SAMPLE_MAX_TRIES = 65536
NO_AGG = 0xFFFFFFFF
SIGAGG_WAVE_MAX = 2048  # BGV_SIGAGG_WAVE_MAX of include/blsgpu.h
MAX_SIGPOOL = 16384  # BGV_MAX_SIGPOOL
SIGPOOL_MAX_BITS = 2048  # BGV_SIGPOOL_MAX_BITS
SIGPOOL_BITS_BYTES = 256  # BGV_SIGPOOL_BITS_BYTES
MAX_SUM_ENTRIES = 64  # BGV_MAX_SUM_ENTRIES
POOL_NOT_ADDED, POOL_ADDED, POOL_KNOWN, POOL_OVERLAP = 0, 1, 2, 3  # BGV_POOL_*

EXPORTED_SYMBOLS = [
    "bgv_init", "bgv_close", "bgv_destroy", "bgv_pubkeys_put", "bgv_pubkeys_count", "bgv_verify",
    "bgv_verify_async", "bgv_aggregate_pubkeys", "bgv_hash_to_g2", "bgv_keygen", "bgv_sign",
    "bgv_set_rng_seed", "bgv_strerror", "bgv_device_count", "bgv_profile",
    "bgv_pubkeys_validate", "bgv_aggregate_signatures", "bgv_deposits_verify", "bgv_set_batching",
    "bgv_verify_partial", "bgv_final_verify", "bgv_debug_prepare", "bgv_debug_uniform", "bgv_set_split",
    "bgv_committee_put", "bgv_committee_drop", "bgv_verify_bits", "bgv_verify_bits_async",
    "bgv_aggregate_committee_bits", "bgv_shuffling_put", "bgv_committee_drop_range",
    "bgv_proposers", "bgv_sync_committee_put", "bgv_proposers_electra", "bgv_sync_committee_put_electra",
    "bgv_verify_spans", "bgv_verify_spans_async", "bgv_aggregate_span",
    "bgv_verify_aggregate", "bgv_verify_aggregate_async", "bgv_debug_sigagg_launches",
    "bgv_sigpool_open", "bgv_sigpool_drop_range", "bgv_sigpool_get", "bgv_verify_accumulate",
    "bgv_verify_accumulate_async", "bgv_debug_sigpool_launches",
    "bgv_sigpool_open_bits", "bgv_verify_accumulate_bits", "bgv_verify_accumulate_bits_async",
    "bgv_sigpool_get_bits", "bgv_sigpool_sum",
]


class BgvSet(ctypes.Structure):
    _fields_ = [
        ("n_pk", ctypes.c_uint32),
        ("sig_len", ctypes.c_uint32),
        ("pk_indices", ctypes.c_void_p),
        ("pk_bytes", ctypes.c_void_p),
        ("msg", ctypes.c_void_p),
        ("sig", ctypes.c_void_p),
    ]


class BgvPkBits(ctypes.Structure):
    _fields_ = [("committee", ctypes.c_uint32), ("n_bits", ctypes.c_uint32), ("bits", ctypes.c_void_p)]


class BgvPkSpan(ctypes.Structure):
    _fields_ = [("committees", ctypes.c_void_p), ("n_committees", ctypes.c_uint32), ("n_bits", ctypes.c_uint32),
                ("bits", ctypes.c_void_p)]


class BgvPoolBits(ctypes.Structure):
    _fields_ = [("n_bits", ctypes.c_uint32), ("bit", ctypes.c_uint32), ("bits", ctypes.c_void_p)]


class BgvPoolGroup(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("n_ids", ctypes.c_uint32)]


class BgvJob(ctypes.Structure):
    _fields_ = [("first_set", ctypes.c_uint32), ("n_sets", ctypes.c_uint32), ("batchable", ctypes.c_uint32)]


class BgvStats(ctypes.Structure):
    _fields_ = [
        ("batch_retries", ctypes.c_uint64),
        ("batch_sigs_success", ctypes.c_uint64),
        ("device_groups", ctypes.c_uint64),
        ("sets_verified", ctypes.c_uint64),
        ("device_ms", ctypes.c_double),
        ("wall_ms", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


DONE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)

_lib = None
_lib_lock = threading.Lock()


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libblsgpu.so; raises if it is missing (no fallback path exists)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError("libblsgpu.so not built (%s): run `python -m lodestar_amd.build`" % path)
        lib = ctypes.CDLL(path)
        P, U32, SZ, I32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int32, ctypes.c_uint64
        sig = {
            "bgv_init": ([P, ctypes.c_int, P], ctypes.c_int),
            "bgv_close": ([P], ctypes.c_int),
            "bgv_destroy": ([P], ctypes.c_int),
            "bgv_pubkeys_put": ([P, U32, P, SZ, ctypes.c_int], ctypes.c_int),
            "bgv_pubkeys_count": ([P], SZ),
            "bgv_verify": ([P, P, SZ, P, SZ, ctypes.c_int, P, P], ctypes.c_int),
            "bgv_verify_async": ([P, P, SZ, P, SZ, ctypes.c_int, P, P, DONE_FN, P], ctypes.c_int),
            "bgv_aggregate_pubkeys": ([P, P, SZ, P], ctypes.c_int),
            "bgv_hash_to_g2": ([P, P, P, SZ, P], ctypes.c_int),
            "bgv_keygen": ([P, P, SZ, ctypes.c_int64, P], ctypes.c_int),
            "bgv_sign": ([P, P, P, SZ, P], ctypes.c_int),
            "bgv_set_rng_seed": ([P, U64], ctypes.c_int),
            "bgv_set_batching": ([P, U32, U32, U32], ctypes.c_int),
            "bgv_set_split": ([P, U32], ctypes.c_int),
            "bgv_verify_partial": ([P, P, SZ, P, P], ctypes.c_int),
            "bgv_final_verify": ([P, P, SZ, P], ctypes.c_int),
            "bgv_debug_prepare": ([P, P, SZ, ctypes.c_int, U64, P, P, P], ctypes.c_int),
            "bgv_debug_uniform": ([P, P, SZ, U64, P, P, SZ, P, P, P], ctypes.c_int),
            "bgv_strerror": ([ctypes.c_int], ctypes.c_char_p),
            "bgv_device_count": ([], ctypes.c_int),
            "bgv_profile": ([P, ctypes.c_int, P, P, ctypes.c_int, P], ctypes.c_int),
            "bgv_pubkeys_validate": ([P, P, SZ, P, P], ctypes.c_int),
            "bgv_aggregate_signatures": ([P, P, P, P, SZ, P, P], ctypes.c_int),
            "bgv_deposits_verify": ([P, P, P, P, SZ, P], ctypes.c_int),
            "bgv_committee_put": ([P, U32, P, SZ], ctypes.c_int),
            "bgv_committee_drop": ([P, U32], ctypes.c_int),
            "bgv_verify_bits": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P], ctypes.c_int),
            "bgv_verify_bits_async": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, DONE_FN, P], ctypes.c_int),
            "bgv_aggregate_committee_bits": ([P, U32, P, U32, P], ctypes.c_int),
            "bgv_shuffling_put": ([P, U32, P, P, SZ, U32, U32, U32, P], ctypes.c_int),
            "bgv_committee_drop_range": ([P, U32, U32], ctypes.c_int),
            "bgv_proposers": ([P, P, U32, P, SZ, P, SZ, U32, U32, P], ctypes.c_int),
            "bgv_sync_committee_put": ([P, U32, P, P, SZ, P, SZ, U32, U32, U32, P, P], ctypes.c_int),
            "bgv_proposers_electra": ([P, P, U32, P, SZ, P, SZ, U32, U32, P], ctypes.c_int),
            "bgv_sync_committee_put_electra": ([P, U32, P, P, SZ, P, SZ, U32, U32, U32, P, P], ctypes.c_int),
            "bgv_verify_spans": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P], ctypes.c_int),
            "bgv_verify_spans_async": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, DONE_FN, P], ctypes.c_int),
            "bgv_aggregate_span": ([P, P, P], ctypes.c_int),
            "bgv_verify_aggregate": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, SZ, P, P, P, P, P], ctypes.c_int),
            "bgv_debug_sigagg_launches": ([P, P], ctypes.c_int),
            "bgv_verify_aggregate_async": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, SZ, P, P, P, P, P, DONE_FN, P],
                                           ctypes.c_int),
            "bgv_sigpool_open": ([P, U32], ctypes.c_int),
            "bgv_sigpool_drop_range": ([P, U32, U32], ctypes.c_int),
            "bgv_sigpool_get": ([P, P, SZ, P, P, P], ctypes.c_int),
            "bgv_verify_accumulate": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, P, P], ctypes.c_int),
            "bgv_verify_accumulate_async": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, P, P, DONE_FN, P], ctypes.c_int),
            "bgv_debug_sigpool_launches": ([P, P], ctypes.c_int),
            "bgv_sigpool_open_bits": ([P, U32, U32], ctypes.c_int),
            "bgv_verify_accumulate_bits": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, P, P, P], ctypes.c_int),
            "bgv_verify_accumulate_bits_async": ([P, P, SZ, P, SZ, P, ctypes.c_int, P, P, P, P, P, DONE_FN, P],
                                                 ctypes.c_int),
            "bgv_sigpool_get_bits": ([P, P, SZ, P, P, P, P, P], ctypes.c_int),
            "bgv_sigpool_sum": ([P, P, SZ, P, P, P, P, SZ, P], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            if name in ("bgv_debug_prepare", "bgv_debug_uniform", "bgv_set_split", "bgv_committee_put",
                        "bgv_committee_drop", "bgv_verify_bits", "bgv_verify_bits_async",
                        "bgv_aggregate_committee_bits", "bgv_shuffling_put",
                        "bgv_committee_drop_range", "bgv_proposers", "bgv_sync_committee_put",
                        "bgv_proposers_electra", "bgv_sync_committee_put_electra",
                        "bgv_verify_spans", "bgv_verify_spans_async", "bgv_aggregate_span",
                        "bgv_verify_aggregate", "bgv_verify_aggregate_async",
                        "bgv_debug_sigagg_launches", "bgv_sigpool_open", "bgv_sigpool_drop_range",
                        "bgv_sigpool_get", "bgv_verify_accumulate", "bgv_verify_accumulate_async",
                        "bgv_debug_sigpool_launches", "bgv_sigpool_open_bits", "bgv_verify_accumulate_bits",
                        "bgv_verify_accumulate_bits_async", "bgv_sigpool_get_bits",
                        "bgv_sigpool_sum") and path != os.path.join(HERE, "libblsgpu.so") and \
                    not hasattr(lib, name):
                continue  # parity hook absent from an older A/B build (tools/gpu/ab.sh)
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = res
        del I32
        _lib = lib
        return lib


def strerror(code: int) -> str:
    return load().bgv_strerror(int(code)).decode()


class BlsGpuError(Exception):
    """Rejection carrying a BLST-style code; str() contains the code name
    (e.g. "BLST_INVALID_SIZE"), like the reference worker's Error(message)."""

    def __init__(self, code: int):
        self.code = abs(int(code))
        super().__init__(strerror(self.code))


class DeviceError(RuntimeError):
    pass


def _check(rc: int):
    if rc < 0:
        if -rc == BGV_E_DEVICE:
            raise DeviceError(strerror(rc))
        raise BlsGpuError(-rc)
    return rc


def _buf(b: bytes):
    return ctypes.create_string_buffer(bytes(b), len(b)) if len(b) else ctypes.create_string_buffer(1)


class Context:
    """One bgv_ctx (device-resident pubkey cache + per-call buffers)."""

    def __init__(self, devices: Optional[Sequence[int]] = None):
        self.lib = load()
        if self.lib.bgv_device_count() <= 0:
            raise DeviceError("no HIP device visible to libblsgpu")
        self._h = ctypes.c_void_p()
        devs = list(devices or [])
        arr = (ctypes.c_int * max(1, len(devs)))(*devs) if devs else None
        _check(self.lib.bgv_init(arr, len(devs), ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self.lib.bgv_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_batching(self, max_batch_slots: int = 0, coalesce_us: int = 0xFFFFFFFF,
                     idle_coalesce_us: int = 0xFFFFFFFF):
        """Super-batch geometry (bgv_set_batching); 0 / 0xFFFFFFFF leave a value unchanged."""
        _check(self.lib.bgv_set_batching(self._h, max_batch_slots, coalesce_us, idle_coalesce_us))

    def set_split(self, min_sets: int):
        """Calls of at least min_sets sets spread over the context's devices (bgv_set_split;
        0 disables)."""
        _check(self.lib.bgv_set_split(self._h, min_sets))

    def verify_packed_one_job(self, packed: "PackedSingleSets", mode: int = MODE_PER_JOB,
                              stats: Optional[BgvStats] = None) -> int:
        """One job over all of a PackedSingleSets' sets (bgv_verify): its code."""
        job = BgvJob(0, packed.nsets, 0)
        out = (ctypes.c_int32 * 1)()
        _check(self.lib.bgv_verify(self._h, ctypes.byref(job), 1, packed.ptr(), packed.nsets, mode, out,
                                   ctypes.byref(stats) if stats is not None else None))
        return out[0]

    def set_rng_seed(self, seed: int):
        _check(self.lib.bgv_set_rng_seed(self._h, seed))

    def profile(self, enable: int = -1):
        """Per-kernel accumulated device ms since the last reset: ({name: ms}, launches);
        enable 1/0 resets and switches event recording on/off, -1 only reads."""
        n = 16
        ms = (ctypes.c_double * n)()
        names = (ctypes.c_char_p * n)()
        launches = ctypes.c_uint64()
        k = _check(self.lib.bgv_profile(self._h, enable, ms, names, n, ctypes.byref(launches)))
        return {names[i].decode(): ms[i] for i in range(k)}, launches.value

    # --- pubkey cache -------------------------------------------------------
    def pubkeys_put(self, first_index: int, keys: bytes, fmt: int = PK_COMPRESSED):
        n = len(keys) // fmt
        assert n * fmt == len(keys)
        _check(self.lib.bgv_pubkeys_put(self._h, first_index, _buf(keys), n, fmt))

    def pubkeys_count(self) -> int:
        return self.lib.bgv_pubkeys_count(self._h)

    # --- device-resident committees (bgv_committee_put) -----------------------
    def committee_put(self, committee_id: int, indices: Sequence[int]):
        """Store a committee's validator indices and their pubkey sum on the device(s) under
        committee_id; sets then name (committee, bitfield): SetSpec(..., committee=, bits=, n_bits=)."""
        arr = (ctypes.c_uint32 * max(1, len(indices)))(*indices)
        _check(self.lib.bgv_committee_put(self._h, committee_id, arr, len(indices)))

    def committee_drop(self, committee_id: int):
        _check(self.lib.bgv_committee_drop(self._h, committee_id))

    def shuffling_put(self, first_id: int, seed: bytes, active_indices: Sequence[int], slots: int,
                      committees_per_slot: int, rounds: int = 90):
        """An epoch's committees in one call (bgv_shuffling_put): the device shuffles active_indices
        (swap-or-not over `rounds` rounds, computeEpochShuffling with unshuffleList), stores the
        slots * committees_per_slot committees under first_id, first_id + 1, ... (an empty one gets
        no id) and sums their pubkeys.  Returns the shuffled indices (numpy uint32 array)."""
        import numpy as np
        assert len(seed) == 32
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        out = np.empty(max(1, act.size), dtype=np.uint32)
        _check(self.lib.bgv_shuffling_put(self._h, first_id, _buf(bytes(seed)), act.ctypes.data, act.size, slots,
                                          committees_per_slot, rounds, out.ctypes.data))
        return out[:act.size]

    def proposers(self, seeds: Sequence[bytes], active_indices: Sequence[int], eff_incr: bytes, max_incr: int = 32,
                  rounds: int = 90) -> list:
        """computeProposerIndex for every 32-byte seed in one call (bgv_proposers): the first
        candidate of each seed accepted by its effective balance (eff_incr: one byte per validator
        index), None where all len(active_indices) candidates were rejected."""
        import numpy as np
        assert all(len(s) == 32 for s in seeds)
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        eff = np.frombuffer(bytes(eff_incr), dtype=np.uint8)
        out = np.empty(max(1, len(seeds)), dtype=np.uint32)
        _check(self.lib.bgv_proposers(self._h, _buf(b"".join(seeds)), len(seeds), act.ctypes.data, act.size,
                                      eff.ctypes.data, eff.size, max_incr, rounds, out.ctypes.data))
        return [None if v == NO_PROPOSER else int(v) for v in out[:len(seeds)]]

    def sync_committee_put(self, committee_id: int, seed: bytes, active_indices: Sequence[int], eff_incr: bytes,
                           max_incr: int = 32, size: int = 512, rounds: int = 90):
        """getNextSyncCommittee in one call (bgv_sync_committee_put): the first `size` candidates
        accepted by balance, repeats kept, become committee committee_id on every device.  Returns
        (indices as a numpy uint32 array, the 48-byte compressed aggregate pubkey)."""
        import numpy as np
        assert len(seed) == 32
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        eff = np.frombuffer(bytes(eff_incr), dtype=np.uint8)
        out = np.empty(max(1, size), dtype=np.uint32)
        agg = ctypes.create_string_buffer(48)
        _check(self.lib.bgv_sync_committee_put(self._h, committee_id, _buf(bytes(seed)), act.ctypes.data, act.size,
                                               eff.ctypes.data, eff.size, max_incr, size, rounds, out.ctypes.data, agg))
        return out[:size], agg.raw

    @staticmethod
    def _eff16(eff_incr16):
        """The Electra balance table as a contiguous uint16 array; values that do not fit are an
        error, never wrapped."""
        import numpy as np
        a = np.asarray(eff_incr16)
        if a.dtype != np.uint16:
            if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 65535):
                raise ValueError("eff_incr16: integers 0..65535 expected")
            a = a.astype(np.uint16)
        return np.ascontiguousarray(a.reshape(-1))

    def proposers_electra(self, seeds: Sequence[bytes], active_indices: Sequence[int], eff_incr16,
                          max_incr: int = 2048, rounds: int = 90) -> list:
        """proposers() under Electra's rule (bgv_proposers_electra, EIP-7251): 16 random bits per
        candidate and eff_incr16, anything convertible to np.uint16, one element per validator
        index (values above 65535 raise ValueError)."""
        import numpy as np
        assert all(len(s) == 32 for s in seeds)
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        eff = self._eff16(eff_incr16)
        out = np.empty(max(1, len(seeds)), dtype=np.uint32)
        _check(self.lib.bgv_proposers_electra(self._h, _buf(b"".join(seeds)), len(seeds), act.ctypes.data, act.size,
                                              eff.ctypes.data, eff.size, max_incr, rounds, out.ctypes.data))
        return [None if v == NO_PROPOSER else int(v) for v in out[:len(seeds)]]

    def sync_committee_put_electra(self, committee_id: int, seed: bytes, active_indices: Sequence[int], eff_incr16,
                                   max_incr: int = 2048, size: int = 512, rounds: int = 90):
        """sync_committee_put() under Electra's rule (bgv_sync_committee_put_electra); eff_incr16 as
        for proposers_electra.  Returns (indices as a numpy uint32 array, the 48-byte aggregate)."""
        import numpy as np
        assert len(seed) == 32
        act = np.ascontiguousarray(active_indices, dtype=np.uint32)
        eff = self._eff16(eff_incr16)
        out = np.empty(max(1, size), dtype=np.uint32)
        agg = ctypes.create_string_buffer(48)
        _check(self.lib.bgv_sync_committee_put_electra(self._h, committee_id, _buf(bytes(seed)), act.ctypes.data,
                                                       act.size, eff.ctypes.data, eff.size, max_incr, size, rounds,
                                                       out.ctypes.data, agg))
        return out[:size], agg.raw

    def committee_drop_range(self, first_id: int, count: int) -> int:
        """Drop the live committees of ids first_id .. first_id + count - 1; returns how many."""
        return _check(self.lib.bgv_committee_drop_range(self._h, first_id, count))

    def aggregate_committee_bits(self, committee_id: int, bits: bytes, n_bits: int) -> bytes:
        """The aggregate of the committee members whose bit is set (SSZ bit order), 96 B
        uncompressed, through the verify path's kernel (bgv_aggregate_committee_bits)."""
        out = ctypes.create_string_buffer(96)
        _check(self.lib.bgv_aggregate_committee_bits(self._h, committee_id, _buf(bits), n_bits, out))
        return out.raw

    def aggregate_span(self, committees: Sequence[int], bits: bytes, n_bits: int) -> bytes:
        """The aggregate of the members one bitfield selects over the listed committees (committee
        c owns the bits from the sum of the lengths before it on), 96 B uncompressed, through the
        verify path's kernel (bgv_aggregate_span)."""
        ids = (ctypes.c_uint32 * max(1, len(committees)))(*committees)
        b = _buf(bits)
        span = BgvPkSpan(ctypes.addressof(ids), len(committees), n_bits, ctypes.addressof(b))
        out = ctypes.create_string_buffer(96)
        _check(self.lib.bgv_aggregate_span(self._h, ctypes.byref(span), out))
        return out.raw

    def keygen(self, sks: bytes, cache_first: int = -1, want_pubkeys: bool = True) -> bytes:
        n = len(sks) // 32
        out = ctypes.create_string_buffer(48 * n) if want_pubkeys else None
        _check(self.lib.bgv_keygen(self._h, _buf(sks), n, cache_first, out))
        return out.raw if want_pubkeys else b""

    def sign(self, sks: bytes, msgs: bytes) -> bytes:
        n = len(sks) // 32
        assert len(msgs) == 32 * n
        out = ctypes.create_string_buffer(96 * n)
        _check(self.lib.bgv_sign(self._h, _buf(sks), _buf(msgs), n, out))
        return out.raw

    # --- parity hooks -------------------------------------------------------
    def aggregate_pubkeys(self, indices: Sequence[int]) -> bytes:
        arr = (ctypes.c_uint32 * max(1, len(indices)))(*indices)
        out = ctypes.create_string_buffer(96)
        _check(self.lib.bgv_aggregate_pubkeys(self._h, arr, len(indices), out))
        return out.raw

    def hash_to_g2(self, msgs: Sequence[bytes]) -> List[bytes]:
        lens = (ctypes.c_uint32 * max(1, len(msgs)))(*[len(m) for m in msgs])
        out = ctypes.create_string_buffer(192 * len(msgs))
        _check(self.lib.bgv_hash_to_g2(self._h, _buf(b"".join(msgs)), lens, len(msgs), out))
        return [out.raw[192 * i:192 * i + 192] for i in range(len(msgs))]

    # --- deposit keys, op-pool aggregation, deposit signatures ----
    def pubkeys_validate(self, keys48: Sequence[bytes]):
        """PublicKey.fromBytes(pk, affine, validate=true) per key -> (codes, uncompressed)."""
        n = len(keys48)
        st = (ctypes.c_int32 * max(1, n))()
        out = ctypes.create_string_buffer(96 * max(1, n))
        _check(self.lib.bgv_pubkeys_validate(self._h, _buf(b"".join(keys48)), n, st, out))
        return list(st[:n]), [out.raw[96 * i:96 * i + 96] for i in range(n)]

    def aggregate_signatures(self, aggregates: Sequence[Sequence[bytes]]):
        """Signature.aggregate over each list of signatures -> [(code, compressed96)]."""
        sigs = [s for agg in aggregates for s in agg]
        counts = (ctypes.c_uint32 * max(1, len(aggregates)))(*[len(a) for a in aggregates])
        lens = (ctypes.c_uint32 * max(1, len(sigs)))(*[len(x) for x in sigs])
        raw = b"".join(bytes(x[:96]).ljust(96, b"\0") for x in sigs)
        out = ctypes.create_string_buffer(96 * max(1, len(aggregates)))
        st = (ctypes.c_int32 * max(1, len(aggregates)))()
        _check(self.lib.bgv_aggregate_signatures(self._h, _buf(raw), lens, counts, len(aggregates), out, st))
        return [(st[a], out.raw[96 * a:96 * a + 96]) for a in range(len(aggregates))]

    def deposits_verify(self, keys48: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes]) -> List[int]:
        n = len(keys48)
        assert len(msgs) == n and len(sigs) == n and all(len(x) == 96 for x in sigs)
        out = (ctypes.c_int32 * max(1, n))()
        _check(self.lib.bgv_deposits_verify(self._h, _buf(b"".join(keys48)), _buf(b"".join(msgs)),
                                            _buf(b"".join(sigs)), n, out))
        return list(out[:n])

    # --- verification -------------------------------------------------------
    def verify_partial(self, sets) -> tuple:
        """One job's shard (list of SetSpec) -> (576-byte Miller-loop product, sig_code, pk_code)
        (bgv_verify_partial)."""
        packed = PackedCall([(list(sets), False)])
        out = ctypes.create_string_buffer(576)
        codes = (ctypes.c_int32 * 2)()
        _check(self.lib.bgv_verify_partial(self._h, packed.sets, packed.nsets, out, codes))
        return out.raw, codes[0], codes[1]

    def verify_partial_packed(self, packed: "PackedSingleSets", lo: int, hi: int) -> tuple:
        """verify_partial over sets [lo, hi) of a PackedSingleSets (no per-set objects)."""
        if not 0 <= lo <= hi <= packed.nsets:
            raise ValueError("shard bounds out of range")
        out = ctypes.create_string_buffer(576)
        codes = (ctypes.c_int32 * 2)()
        _check(self.lib.bgv_verify_partial(self._h, packed.ptr(lo), hi - lo, out, codes))
        return out.raw, codes[0], codes[1]

    def debug_prepare(self, sets, path: int, seed: int = 1):
        """bgv_debug_prepare (parity hook): per set (H(m) 192 B, f 576 B, sig status,
        pk status) from the bulk (PATH_BULK) or latency (PATH_LATENCY) kernels."""
        packed = PackedCall([(list(sets), False)])
        n = packed.nsets
        h = ctypes.create_string_buffer(192 * max(1, n))
        f = ctypes.create_string_buffer(576 * max(1, n))
        st = (ctypes.c_int32 * max(2, 2 * n))()
        _check(self.lib.bgv_debug_prepare(self._h, packed.sets, n, path, seed, h, f, st))
        return [(h.raw[192 * i:192 * i + 192], f.raw[576 * i:576 * i + 576], st[2 * i], st[2 * i + 1])
                for i in range(n)]

    def debug_uniform(self, sets, seed: int, tests=()):
        """bgv_debug_uniform (parity hook): one uniform group of the sets (one signing root) and
        retry tests over it, tests = [(slot mask, weighted)].  Returns (MillerLoop(sum r_i pk_i, H),
        [(test's pubkey-sum pair, test's signature pair)]), 576 B each."""
        packed = PackedCall([(list(sets), False)])
        n, nt = packed.nsets, len(tests)
        masks = (ctypes.c_uint64 * max(1, nt))(*[m for m, _ in tests])
        wts = (ctypes.c_uint32 * max(1, nt))(*[1 if w else 0 for _, w in tests])
        first = ctypes.create_string_buffer(576)
        pk = ctypes.create_string_buffer(576 * max(1, nt))
        sig = ctypes.create_string_buffer(576 * max(1, nt))
        _check(self.lib.bgv_debug_uniform(self._h, packed.sets, n, seed, masks, wts, nt, first, pk, sig))
        return first.raw, [(pk.raw[576 * t:576 * t + 576], sig.raw[576 * t:576 * t + 576]) for t in range(nt)]

    def final_verify(self, partials: Sequence[bytes]) -> bool:
        """Product of serialized partials and one final exponentiation == 1 (bgv_final_verify)."""
        v = ctypes.c_int32()
        _check(self.lib.bgv_final_verify(self._h, _buf(b"".join(partials)), len(partials), ctypes.byref(v)))
        return v.value == 1

    def verify_jobs(self, jobs, mode: int = MODE_WORKER, stats: Optional[BgvStats] = None) -> List[int]:
        """jobs: list of (sets, batchable) with sets = list of SetSpec.  Returns the
        per-job codes (1 valid, 0 invalid, -code error)."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        njobs = len(packed.jobs_in)
        out = (ctypes.c_int32 * max(1, njobs))()
        st = ctypes.byref(stats) if stats is not None else None
        if packed.spans is not None:  # some set names several committees under one bitfield
            rc = self.lib.bgv_verify_spans(self._h, packed.jobs, njobs, packed.sets, packed.nsets, packed.spans,
                                           mode, out, st)
        elif packed.pkbits is not None:  # some set names (committee, bitfield)
            rc = self.lib.bgv_verify_bits(self._h, packed.jobs, njobs, packed.sets, packed.nsets, packed.pkbits,
                                          mode, out, st)
        else:
            rc = self.lib.bgv_verify(self._h, packed.jobs, njobs, packed.sets, packed.nsets, mode, out, st)
        _check(rc)
        return list(out[:njobs])

    def verify_jobs_async(self, jobs, mode: int = MODE_WORKER) -> "PendingVerify":
        """verify_jobs through the asynchronous entry point of the call's form (bgv_verify_async,
        bgv_verify_bits_async or bgv_verify_spans_async): the call is queued when this returns, so
        calls submitted from one thread are queued in that order.  Returns a PendingVerify whose
        wait() gives what verify_jobs returns."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        return PendingVerify(self, packed, mode)

    def verify_aggregate(self, jobs, agg_of_set: Sequence[int], naggs: int, mode: int = MODE_WORKER,
                         stats: Optional[BgvStats] = None):
        """bgv_verify_aggregate: verify_jobs whose call also sums the signatures it accepted.
        agg_of_set[i] is the aggregate of set i (in job order; < naggs) or NO_AGG.  Returns
        (codes, [(status, count, compressed96)])."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(agg_of_set) != packed.nsets:
            raise ValueError("agg_of_set takes one entry per set")
        njobs = len(packed.jobs_in)
        out = (ctypes.c_int32 * max(1, njobs))()
        tags = (ctypes.c_uint32 * max(1, packed.nsets))(*agg_of_set)
        agg = ctypes.create_string_buffer(96 * max(1, naggs))
        ast = (ctypes.c_int32 * max(1, naggs))()
        cnt = (ctypes.c_uint32 * max(1, naggs))()
        st = ctypes.byref(stats) if stats is not None else None
        _check(self.lib.bgv_verify_aggregate(self._h, packed.jobs, njobs, packed.sets, packed.nsets,
                                             packed.as_spans(), mode, tags, naggs, out, agg, ast, cnt, st))
        return list(out[:njobs]), [(ast[a], cnt[a], agg.raw[96 * a:96 * a + 96]) for a in range(naggs)]

    def sigagg_launches(self):
        """bgv_debug_sigagg_launches (parity hook): aggregation steps launched so far with the
        (wavefront, lane) decoding form."""
        out = (ctypes.c_uint64 * 2)()
        _check(self.lib.bgv_debug_sigagg_launches(self._h, out))
        return out[0], out[1]

    def verify_aggregate_async(self, jobs, agg_of_set: Sequence[int], naggs: int, mode: int = MODE_WORKER):
        """bgv_verify_aggregate_async: returns a PendingAggregate whose wait() gives what
        verify_aggregate returns, as the outputs stood when done() fired."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(agg_of_set) != packed.nsets:
            raise ValueError("agg_of_set takes one entry per set")
        return PendingAggregate(self, packed, agg_of_set, naggs, mode)

    # --- device-resident signature pools (bgv_sigpool_open) --------------------
    def sigpool_open(self, pool_id: int, n_bits: int = 0):
        """Open pool entry pool_id (0 .. MAX_SIGPOOL - 1): a G2 accumulator, empty, with a count;
        with n_bits (1 .. SIGPOOL_MAX_BITS) also a participation field of that many positions, all
        clear (bgv_sigpool_open_bits)."""
        if n_bits:
            _check(self.lib.bgv_sigpool_open_bits(self._h, pool_id, n_bits))
        else:
            _check(self.lib.bgv_sigpool_open(self._h, pool_id))

    def sigpool_drop_range(self, first_id: int, count: int) -> int:
        """Drop the live entries of ids first_id .. first_id + count - 1; returns how many."""
        return _check(self.lib.bgv_sigpool_drop_range(self._h, first_id, count))

    def sigpool_get(self, ids: Sequence[int]):
        """bgv_sigpool_get: [(status, count, compressed96)] per id, entries unchanged."""
        n = len(ids)
        arr = (ctypes.c_uint32 * max(1, n))(*ids)
        out = ctypes.create_string_buffer(96 * max(1, n))
        cnt = (ctypes.c_uint32 * max(1, n))()
        st = (ctypes.c_int32 * max(1, n))()
        _check(self.lib.bgv_sigpool_get(self._h, arr, n, out, cnt, st))
        return [(st[k], cnt[k], out.raw[96 * k:96 * k + 96]) for k in range(n)]

    def verify_accumulate(self, jobs, pool_of_set: Sequence[int], mode: int = MODE_WORKER,
                          stats: Optional[BgvStats] = None):
        """bgv_verify_accumulate: verify_jobs whose accepted signatures are added to pool entries.
        pool_of_set[i] is the entry of set i (in job order) or NO_AGG.  Returns (codes, added) with
        added[i] True iff set i was added."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(pool_of_set) != packed.nsets:
            raise ValueError("pool_of_set takes one entry per set")
        njobs = len(packed.jobs_in)
        out = (ctypes.c_int32 * max(1, njobs))()
        tags = (ctypes.c_uint32 * max(1, packed.nsets))(*pool_of_set)
        added = (ctypes.c_uint8 * max(1, packed.nsets))()
        st = ctypes.byref(stats) if stats is not None else None
        _check(self.lib.bgv_verify_accumulate(self._h, packed.jobs, njobs, packed.sets, packed.nsets,
                                              packed.as_spans(), mode, tags, out, added, st))
        return list(out[:njobs]), [bool(a) for a in added[:packed.nsets]]

    def verify_accumulate_async(self, jobs, pool_of_set: Sequence[int], mode: int = MODE_WORKER):
        """bgv_verify_accumulate_async: returns a PendingAccumulate whose wait() gives what
        verify_accumulate returns; the additions are visible to sigpool_get once it has returned."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(pool_of_set) != packed.nsets:
            raise ValueError("pool_of_set takes one entry per set")
        return PendingAccumulate(self, packed, pool_of_set, mode)

    def verify_accumulate_bits(self, jobs, pool_of_set: Sequence[int], bits_of_set, mode: int = MODE_WORKER,
                               stats: Optional[BgvStats] = None):
        """bgv_verify_accumulate_bits: verify_accumulate into entries that hold participation bits.
        bits_of_set is None (no entry with bits is tagged) or one item per set: None (the set's
        entry is plain, or the set is untagged), (n_bits, position) for a single member or (n_bits,
        field bytes) in SSZ bit order.  Returns (codes, outcome) with outcome[i] one of POOL_*."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(pool_of_set) != packed.nsets:
            raise ValueError("pool_of_set takes one entry per set")
        njobs = len(packed.jobs_in)
        out = (ctypes.c_int32 * max(1, njobs))()
        tags = (ctypes.c_uint32 * max(1, packed.nsets))(*pool_of_set)
        bits, _keep = pack_poolbits(bits_of_set, packed.nsets)
        outcome = (ctypes.c_uint8 * max(1, packed.nsets))()
        st = ctypes.byref(stats) if stats is not None else None
        _check(self.lib.bgv_verify_accumulate_bits(self._h, packed.jobs, njobs, packed.sets, packed.nsets,
                                                   packed.as_spans(), mode, tags, bits, out, outcome, st))
        return list(out[:njobs]), list(outcome[:packed.nsets])

    def verify_accumulate_bits_async(self, jobs, pool_of_set: Sequence[int], bits_of_set, mode: int = MODE_WORKER):
        """bgv_verify_accumulate_bits_async: returns a PendingAccumulate whose wait() gives what
        verify_accumulate_bits returns."""
        packed = jobs if isinstance(jobs, PackedCall) else PackedCall(jobs)
        if len(pool_of_set) != packed.nsets:
            raise ValueError("pool_of_set takes one entry per set")
        return PendingAccumulate(self, packed, pool_of_set, mode, bits_of_set=bits_of_set, with_bits=True)

    def sigpool_get_bits(self, ids: Sequence[int]):
        """bgv_sigpool_get_bits: [(status, count, compressed96, n_bits, field)] per id, field being
        the ceil(n_bits / 8) bytes of the entry's positions (b"" for a plain or not-live entry)."""
        n = len(ids)
        arr = (ctypes.c_uint32 * max(1, n))(*ids)
        out = ctypes.create_string_buffer(96 * max(1, n))
        cnt = (ctypes.c_uint32 * max(1, n))()
        st = (ctypes.c_int32 * max(1, n))()
        bits = ctypes.create_string_buffer(SIGPOOL_BITS_BYTES * max(1, n))
        nb = (ctypes.c_uint32 * max(1, n))()
        _check(self.lib.bgv_sigpool_get_bits(self._h, arr, n, out, cnt, st, bits, nb))
        return [(st[k], cnt[k], out.raw[96 * k:96 * k + 96], nb[k],
                 bits.raw[SIGPOOL_BITS_BYTES * k:SIGPOOL_BITS_BYTES * k + (nb[k] + 7) // 8]) for k in range(n)]

    def sigpool_sum(self, groups: Sequence[Sequence[int]], with_bits: bool = True, bits_stride: Optional[int] = None):
        """bgv_sigpool_sum: per group of entry ids [(status, count, compressed96, n_bits, field)],
        the G2 sum of the entries and their fields concatenated in list order; entries unchanged.
        with_bits=False passes no bits buffer (n_bits is still returned, field is b"").  The stride
        defaults to the largest a group of its length can need."""
        ng = len(groups)
        arrs = [(ctypes.c_uint32 * max(1, len(g)))(*g) for g in groups]
        gs = (BgvPoolGroup * max(1, ng))()
        for k, g in enumerate(groups):
            gs[k].ids = ctypes.cast(arrs[k], ctypes.c_void_p)
            gs[k].n_ids = len(g)
        if bits_stride is None:
            bits_stride = SIGPOOL_BITS_BYTES * max([1] + [min(len(g), MAX_SUM_ENTRIES) for g in groups])
        out = ctypes.create_string_buffer(96 * max(1, ng))
        cnt = (ctypes.c_uint32 * max(1, ng))()
        st = (ctypes.c_int32 * max(1, ng))()
        nb = (ctypes.c_uint32 * max(1, ng))()
        bits = ctypes.create_string_buffer(max(1, bits_stride * ng)) if with_bits else None
        _check(self.lib.bgv_sigpool_sum(self._h, gs, ng, out, cnt, st, bits, bits_stride, nb))
        return [(st[k], cnt[k], out.raw[96 * k:96 * k + 96], nb[k],
                 bits.raw[bits_stride * k:bits_stride * k + (nb[k] + 7) // 8] if with_bits else b"")
                for k in range(ng)]

    def sigpool_launches(self):
        """bgv_debug_sigpool_launches (parity hook): accumulation steps launched so far with the
        (wavefront, lane) decoding form."""
        out = (ctypes.c_uint64 * 2)()
        _check(self.lib.bgv_debug_sigpool_launches(self._h, out))
        return out[0], out[1]


class PendingVerify:
    """One bgv_verify_async / bgv_verify_bits_async / bgv_verify_spans_async call: keeps its
    buffers and its callback alive until done() has fired on one of the context's threads (or, for
    a call the host's checks decide alone, inside the submit), where the codes are read.  `stats`
    is the call's BgvStats, filled before done()."""

    def __init__(self, ctx: "Context", packed: "PackedCall", mode: int):
        self._packed = packed
        njobs = len(packed.jobs_in)
        self._out = (ctypes.c_int32 * max(1, njobs))()
        self.stats = BgvStats()
        self._event = threading.Event()
        self._rc = None
        self._result = None

        def done(_user, rc):
            self._rc = rc
            self._result = list(self._out[:njobs])
            self._event.set()

        self._done = DONE_FN(done)
        st = ctypes.byref(self.stats)
        if packed.spans is not None:  # the entry point of the call's form, as verify_jobs picks it
            rc = ctx.lib.bgv_verify_spans_async(ctx.handle, packed.jobs, njobs, packed.sets, packed.nsets,
                                                packed.spans, mode, self._out, st, self._done, None)
        elif packed.pkbits is not None:
            rc = ctx.lib.bgv_verify_bits_async(ctx.handle, packed.jobs, njobs, packed.sets, packed.nsets,
                                               packed.pkbits, mode, self._out, st, self._done, None)
        else:
            rc = ctx.lib.bgv_verify_async(ctx.handle, packed.jobs, njobs, packed.sets, packed.nsets, mode,
                                          self._out, st, self._done, None)
        _check(rc)

    def wait(self, timeout: Optional[float] = None) -> List[int]:
        if not self._event.wait(timeout):
            raise TimeoutError("bgv_verify_async: done() has not fired")
        _check(self._rc)
        return self._result


class PendingAggregate:
    """One bgv_verify_aggregate_async call: keeps its buffers alive until done() has fired on the
    context's worker thread, where the outputs are read."""

    def __init__(self, ctx: "Context", packed: "PackedCall", agg_of_set: Sequence[int], naggs: int, mode: int):
        self._packed = packed
        njobs = len(packed.jobs_in)
        self._out = (ctypes.c_int32 * max(1, njobs))()
        self._tags = (ctypes.c_uint32 * max(1, packed.nsets))(*agg_of_set)
        self._agg = ctypes.create_string_buffer(96 * max(1, naggs))
        self._ast = (ctypes.c_int32 * max(1, naggs))()
        self._cnt = (ctypes.c_uint32 * max(1, naggs))()
        self.stats = BgvStats()
        self._event = threading.Event()
        self._rc = None
        self._result = None

        def done(_user, rc):
            self._rc = rc
            self._result = (list(self._out[:njobs]),
                            [(self._ast[a], self._cnt[a], self._agg.raw[96 * a:96 * a + 96]) for a in range(naggs)])
            self._event.set()

        self._done = DONE_FN(done)
        _check(ctx.lib.bgv_verify_aggregate_async(ctx.handle, packed.jobs, njobs, packed.sets, packed.nsets,
                                                  packed.as_spans(), mode, self._tags, naggs, self._out, self._agg,
                                                  self._ast, self._cnt, ctypes.byref(self.stats), self._done, None))

    def wait(self, timeout: Optional[float] = None):
        if not self._event.wait(timeout):
            raise TimeoutError("bgv_verify_aggregate_async: done() has not fired")
        _check(self._rc)
        return self._result


class PendingAccumulate:
    """One bgv_verify_accumulate_async call: keeps its buffers alive until done() has fired on the
    context's worker thread, where the outputs are read."""

    def __init__(self, ctx: "Context", packed: "PackedCall", pool_of_set: Sequence[int], mode: int,
                 bits_of_set=None, with_bits: bool = False):
        self._packed = packed
        njobs, nsets = len(packed.jobs_in), packed.nsets
        self._out = (ctypes.c_int32 * max(1, njobs))()
        self._tags = (ctypes.c_uint32 * max(1, nsets))(*pool_of_set)
        self._added = (ctypes.c_uint8 * max(1, nsets))()
        self.stats = BgvStats()
        self._event = threading.Event()
        self._rc = None
        self._result = None

        def done(_user, rc):
            self._rc = rc
            self._result = (list(self._out[:njobs]),
                            list(self._added[:nsets]) if with_bits else [bool(a) for a in self._added[:nsets]])
            self._event.set()

        self._done = DONE_FN(done)
        if with_bits:  # the fields are copied at submit: nothing of them is kept here
            bits, _keep = pack_poolbits(bits_of_set, nsets)
            _check(ctx.lib.bgv_verify_accumulate_bits_async(ctx.handle, packed.jobs, njobs, packed.sets, nsets,
                                                            packed.as_spans(), mode, self._tags, bits, self._out,
                                                            self._added, ctypes.byref(self.stats), self._done, None))
            return
        _check(ctx.lib.bgv_verify_accumulate_async(ctx.handle, packed.jobs, njobs, packed.sets, nsets,
                                                   packed.as_spans(), mode, self._tags, self._out, self._added,
                                                   ctypes.byref(self.stats), self._done, None))

    def wait(self, timeout: Optional[float] = None):
        if not self._event.wait(timeout):
            raise TimeoutError("bgv_verify_accumulate_async: done() has not fired")
        _check(self._rc)
        return self._result


def pack_poolbits(bits_of_set, nsets: int):
    """bits_of_set (Context.verify_accumulate_bits) as a bgv_poolbits array, or None; the second
    value keeps the field buffers alive."""
    if bits_of_set is None:
        return None, None
    if len(bits_of_set) != nsets:
        raise ValueError("bits_of_set takes one entry per set")
    arr = (BgvPoolBits * max(1, nsets))()
    keep = []
    for k, item in enumerate(bits_of_set):
        if item is None:
            continue
        n_bits, member = item
        arr[k].n_bits = n_bits
        if isinstance(member, int):
            arr[k].bit = member
        else:
            buf = ctypes.create_string_buffer(bytes(member), max(1, len(member)))
            keep.append(buf)
            arr[k].bits = ctypes.cast(buf, ctypes.c_void_p)
    return arr, keep


class SetSpec:
    """One ISignatureSet in C-ABI terms: pubkeys by cache index, as 96-B bytes, or as the members
    of a device-resident committee (Context.committee_put) selected by an SSZ bitfield of n_bits
    bits (member k takes part iff (bits[k >> 3] >> (k & 7)) & 1).  committees=[ids] lays the one
    bitfield over several committees, concatenated in list order (bgv_pkspan); a list of one id is
    committee=id."""

    __slots__ = ("pk_indices", "pk_bytes", "msg", "sig", "committee", "committees", "bits", "n_bits")

    def __init__(self, msg: bytes, sig: bytes, pk_indices: Optional[Sequence[int]] = None,
                 pk_bytes: Optional[Sequence[bytes]] = None, committee: Optional[int] = None,
                 bits: Optional[bytes] = None, n_bits: Optional[int] = None,
                 committees: Optional[Sequence[int]] = None):
        if committees is not None:
            if committee is not None or len(committees) == 0:
                raise ValueError("committees takes at least one id, and no committee beside it")
            committees = [int(c) for c in committees]
            committee = committees[0]  # the checks below; a list of one id is that committee set
        self.committees = committees if committees is not None and len(committees) > 1 else None
        self.pk_indices = list(pk_indices) if pk_indices is not None else None
        self.pk_bytes = list(pk_bytes) if pk_bytes is not None else None
        self.msg = bytes(msg)
        self.sig = bytes(sig)
        self.committee = committee
        self.bits = bytes(bits) if bits is not None else None
        self.n_bits = n_bits
        if committee is not None:
            if pk_indices is not None or pk_bytes is not None or bits is None or n_bits is None:
                raise ValueError("a committee set takes bits and n_bits, and no pk_indices / pk_bytes")
            if len(self.bits) != (n_bits + 7) // 8:
                raise ValueError("bits must hold ceil(n_bits / 8) bytes")
        elif (self.pk_indices is None) == (self.pk_bytes is None):
            raise ValueError("exactly one of pk_indices / pk_bytes")

    @property
    def n_pk(self):
        if self.committee is not None:
            return sum(bin(b).count("1") for b in self.bits)
        return len(self.pk_indices) if self.pk_indices is not None else len(self.pk_bytes)


class PackedSingleSets:
    """n single-pubkey sets over contiguous buffers (no per-set Python objects): set i has
    signing root msgs[32 i:32 i + 32], signature sigs[96 i:96 i + 96] and cached pubkey index
    idx[i].  For bulk shards (the config-5 epoch sweep: 2^20 sets) where SetSpec lists would
    cost seconds of host time.  `sets` / `nsets` / `slice(lo, hi)` feed bgv_verify_partial."""

    def __init__(self, msgs: bytes, sigs: bytes, idx: Sequence[int]):
        import numpy as np
        n = len(idx)
        if len(msgs) != 32 * n or len(sigs) != 96 * n:
            raise ValueError("msgs / sigs sizes do not match the index count")
        self._msg = np.frombuffer(bytes(msgs), dtype=np.uint8).copy()
        self._sig = np.frombuffer(bytes(sigs), dtype=np.uint8).copy()
        self._idx = np.asarray(idx, dtype=np.uint32).copy()
        rec = np.dtype([("n_pk", "<u4"), ("sig_len", "<u4"), ("pk_indices", "<u8"), ("pk_bytes", "<u8"),
                        ("msg", "<u8"), ("sig", "<u8")])
        assert rec.itemsize == ctypes.sizeof(BgvSet)
        arr = np.zeros(max(1, n), dtype=rec)
        k = np.arange(n, dtype=np.uint64)
        arr["n_pk"][:n] = 1
        arr["sig_len"][:n] = 96
        arr["pk_indices"][:n] = self._idx.ctypes.data + 4 * k
        arr["msg"][:n] = self._msg.ctypes.data + 32 * k
        arr["sig"][:n] = self._sig.ctypes.data + 96 * k
        self._arr = arr
        self.nsets = n

    def ptr(self, lo: int = 0):
        return ctypes.c_void_p(self._arr.ctypes.data + lo * ctypes.sizeof(BgvSet))


class PackedCall:
    """Keeps every buffer of one bgv_verify call alive and builds the C arrays."""

    def as_spans(self):
        """The call's bgv_pkspan array (None for plain sets): a (committee, bitfield) set is the
        span over that one committee."""
        if self.spans is not None or self.pkbits is None:
            return self.spans
        spans = (BgvPkSpan * max(1, self.nsets))()  # zeroed: n_committees = 0
        for i in range(self.nsets):
            if self.pkbits[i].committee == NO_COMMITTEE:
                continue
            one = (ctypes.c_uint32 * 1)(self.pkbits[i].committee)
            self._keep.append(one)
            spans[i].committees = ctypes.addressof(one)
            spans[i].n_committees = 1
            spans[i].n_bits = self.pkbits[i].n_bits
            spans[i].bits = self.pkbits[i].bits
        self.spans = spans
        return spans

    def __init__(self, jobs):
        all_sets = []
        jarr = (BgvJob * max(1, len(jobs)))()
        for j, (sets, batchable) in enumerate(jobs):
            jarr[j].first_set = len(all_sets)
            jarr[j].n_sets = len(sets)
            jarr[j].batchable = 1 if batchable else 0
            all_sets.extend(sets)
        self.jobs_in = jobs
        self.nsets = len(all_sets)
        sarr = (BgvSet * max(1, len(all_sets)))()
        keep = []
        # the bgv_pkbits array beside the sets, only when some set names a committee
        # ... or the bgv_pkspan array, when some set names more than one committee
        self.pkbits = self.spans = None
        if any(s.committees is not None for s in all_sets):
            self.spans = (BgvPkSpan * max(1, len(all_sets)))()  # zeroed: n_committees = 0
        elif any(s.committee is not None for s in all_sets):
            self.pkbits = (BgvPkBits * max(1, len(all_sets)))()
            for i in range(len(all_sets)):
                self.pkbits[i].committee = NO_COMMITTEE
        for i, s in enumerate(all_sets):
            msg = ctypes.create_string_buffer(s.msg, 32) if len(s.msg) == 32 else None
            if msg is None:
                raise ValueError("signing root must be 32 bytes")
            sig = _buf(s.sig)
            keep += [msg, sig]
            sarr[i].n_pk = s.n_pk
            sarr[i].sig_len = len(s.sig)
            sarr[i].msg = ctypes.addressof(msg)
            sarr[i].sig = ctypes.addressof(sig)
            if s.committee is not None:
                bits = _buf(s.bits)
                keep.append(bits)
                if self.spans is not None:
                    ids = s.committees if s.committees is not None else [s.committee]
                    arr = (ctypes.c_uint32 * len(ids))(*ids)
                    keep.append(arr)
                    self.spans[i].committees = ctypes.addressof(arr)
                    self.spans[i].n_committees = len(ids)
                    self.spans[i].n_bits = s.n_bits
                    self.spans[i].bits = ctypes.addressof(bits)
                else:
                    self.pkbits[i].committee = s.committee
                    self.pkbits[i].n_bits = s.n_bits
                    self.pkbits[i].bits = ctypes.addressof(bits)
            elif s.pk_indices is not None:
                idx = (ctypes.c_uint32 * max(1, len(s.pk_indices)))(*s.pk_indices)
                keep.append(idx)
                sarr[i].pk_indices = ctypes.addressof(idx)
            else:
                pkb = _buf(b"".join(s.pk_bytes))
                keep.append(pkb)
                sarr[i].pk_bytes = ctypes.addressof(pkb)
        self.jobs, self.sets, self._keep = jarr, sarr, keep
