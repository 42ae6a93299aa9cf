"""ctypes binding of libdpt.so (include/dpt.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is
visible, every call raises ``DptError``.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPT_LIB") or os.path.join(HERE, "libdpt.so")

DPT_OK = 0
DPT_E_VOCAB = -3
DPT_E_CAP = -4
DPT_E_RCCL = -6
DPT_RCCL_ID_BYTES = 128
DPT_MODE_RAW = 0
DPT_MODE_PRESPLIT = 1
DPT_MODE_ATOMS = 2
DPT_FLAG_UNCAPPED = 0x10
DPT_FLAG_LEN_ONLY = 0x20
STATUS_OK, STATUS_NO_TOKENIZATION, STATUS_EMPTY_WORD, STATUS_TOO_LONG, STATUS_INTERNAL = range(5)
DPT_DETOK_PIECES, DPT_DETOK_SP, DPT_DETOK_BYTELEVEL = range(3)
DPT_DECODE_STRIP_SPACE = 1
DPT_HOST_LAYOUT_SEGS = 7
RT_EQUAL, RT_DIFFERS = 0, 5
PRETOK_NEEDS_HOST = 6
DPT_E_ARG = -1


class DptError(RuntimeError):
    pass


class VocabStats(ctypes.Structure):
    _fields_ = [("n_tokens", ctypes.c_uint32), ("n_nodes", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("max_bytes", ctypes.c_uint32), ("max_cp", ctypes.c_uint32), ("device_bytes", ctypes.c_uint64),
                ("hash_max_probe", ctypes.c_uint32), ("hash_buckets", ctypes.c_uint32)]


class CollateOpts(ctypes.Structure):
    """dpt_collate_opts"""
    _fields_ = [("row_len", ctypes.c_uint32), ("row_stride", ctypes.c_uint64), ("pad_id", ctypes.c_int32),
                ("bos_id", ctypes.c_int32), ("eos_id", ctypes.c_int32), ("ignore_id", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


COLLATE_BOS, COLLATE_EOS, COLLATE_PAD_LEFT, COLLATE_TRUNC_LEFT, COLLATE_I64 = 1, 2, 4, 8, 16
COLLATE_SEP, COLLATE_MASK_A, COLLATE_TRIM_A_FIRST = 32, 64, 128   # dpt_collate_pair only
PACK_MASK_FIRST = 256   # dpt_pack_write only
PACK_NONE = 0xFFFFFFFF


class CollateSide(ctypes.Structure):
    """dpt_collate_side: device addresses (0 = NULL)"""
    _fields_ = [("ids", ctypes.c_void_p), ("off", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class WordSide(ctypes.Structure):
    """dpt_word_side: device addresses (0 = NULL)"""
    _fields_ = [("off", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("status", ctypes.c_void_p), ("tok_word", ctypes.c_void_p),
                ("tok_end", ctypes.c_void_p)]


WORDS_LESS, WORDS_GREATER = 1, 2


class CollatePairOpts(ctypes.Structure):
    """dpt_collate_pair_opts"""
    _fields_ = [("row_len", ctypes.c_uint32), ("row_stride", ctypes.c_uint64), ("pad_id", ctypes.c_int32),
                ("bos_id", ctypes.c_int32), ("sep_id", ctypes.c_int32), ("eos_id", ctypes.c_int32),
                ("ignore_id", ctypes.c_int32), ("max_a", ctypes.c_uint32), ("max_b", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


_lib = None
P = ctypes.c_void_p
U64 = ctypes.c_uint64
I32 = ctypes.c_int
U32 = ctypes.c_uint32

PP, PU64 = ctypes.POINTER(P), ctypes.POINTER(U64)

# include/dpt.h: every exported call, name -> (restype, argtypes).  lib() binds from this table alone.
CALLS = {
    "dpt_last_error": (ctypes.c_char_p, []),
    "dpt_abi_version": (I32, []),
    "dpt_vocab_create": (I32, [P, P, P, U32, I32, PP]),
    "dpt_vocab_destroy": (I32, [P]),
    "dpt_vocab_stats_get": (I32, [P, ctypes.POINTER(VocabStats)]),
    "dpt_ctx_create": (I32, [I32, PP]),
    "dpt_ctx_destroy": (I32, [P]),
    "dpt_ctx_reserve": (I32, [P, U64, U64]),
    "dpt_ctx_reserve_vocab": (I32, [P, P, U64, U64, U64]),
    "dpt_ctx_workspace_bytes": (I32, [P, PU64, PU64]),
    "dpt_ctx_long_need": (I32, [P, PU64, PU64]),
    "dpt_encode": (I32, [P, P, I32, P, U64, P, P, U64, P, U64, P, P, P, P]),
    "dpt_encode_host": (I32, [P, P, I32, P, U64, P, P, U64, P, U64, P, P, P]),
    "dpt_encode_padded": (I32, [P, P, I32, P, U64, P, P, U64, P, U64, P, P, P, P]),
    "dpt_dp_host": (I32, [P, P, I32, P, U64, P, P, U64, P, P, P]),
    "dpt_dp_host_far": (I32, [P, P, I32, P, U64, P, P, U64, P, P, P, P, U64, P]),
    "dpt_token_histogram": (I32, [P, P, U64, P, U32, P]),
    "dpt_token_spans": (I32, [P, I32, P, U64, P, P, U64, P, P, P, P, P, P, P]),
    "dpt_token_spans_host": (I32, [P, P, I32, P, U64, P, P, U64, P, P, P, P, P, P]),
    "dpt_ctx_set_histogram": (I32, [P, P, U32]),
    "dpt_ctx_set_histogram_ex": (I32, [P, P, U32, I32]),
    "dpt_ctx_profile": (I32, [P, I32]),
    "dpt_ctx_profile_read": (I32, [P, ctypes.POINTER(ctypes.c_double), PU64]),
    "dpt_ctx_debug_counter_bias": (I32, [P, U64]),
    "dpt_debug_launch_plan": (I32, [I32] * 8 + [U64, I32, U32, U32, ctypes.POINTER(I32)]),
    "dpt_debug_launch_plan_lean": (I32, [I32] * 6 + [U64, U32, ctypes.POINTER(I32)]),
    "dpt_ctx_debug_lean_words": (I32, [P, ctypes.POINTER(U32)]),
    "dpt_ctx_debug_no_lean": (I32, [P, I32]),
    "dpt_debug_vocab_table": (I32, [P, P, P, U32, I32, P, U64, PU64]),
    "dpt_debug_host_layout": (I32, [I32, U64, U64, U64, I32, U64, PU64]),
    "dpt_debug_wave_grid": (I32, [U64, U32, ctypes.POINTER(U32)]),
    "dpt_rccl_get_unique_id": (I32, [P]),
    "dpt_rccl_comm_create": (I32, [P, I32, I32, I32, PP]),
    "dpt_rccl_comm_destroy": (I32, [P]),
    "dpt_hist_allreduce": (I32, [P, ctypes.c_size_t, P, P]),
    # "Decode"
    "dpt_detok_create": (I32, [P, P, P, U32, I32, P, U32, I32, PP]),
    "dpt_detok_destroy": (I32, [P]),
    "dpt_decode_sizes": (I32, [P, P, P, P, U64, I32, P, P]),
    "dpt_decode": (I32, [P, P, P, P, U64, I32, P, P, P, P]),
    "dpt_roundtrip": (I32, [P, P, P, P, P, P, U64, I32, P, P, P]),
    "dpt_decode_host": (I32, [P, P, P, P, P, U64, I32, P, U64, P, P]),
    "dpt_roundtrip_host": (I32, [P, P, P, P, P, P, P, U64, I32, P, P]),
    "dpt_debug_detok_table": (I32, [P, P, P, U32, I32, P, U32, I32, P, U64, PU64]),
    # model-input batches
    "dpt_collate": (I32, [P, P, P, P, U64, ctypes.POINTER(CollateOpts), P, P, P, P, P]),
    "dpt_collate_pair": (I32, [ctypes.POINTER(CollateSide), ctypes.POINTER(CollateSide), U64, ctypes.POINTER(CollatePairOpts),
                               P, P, P, P, P, P, P]),
    # llama-mode pre-tokenization on the device
    "dpt_pretok_create": (I32, [P, P, U32, P, U32, P, P, U32, I32, PP]),
    "dpt_pretok_destroy": (I32, [P]),
    "dpt_pretok_sizes": (I32, [P, P, P, U64, P, P, P]),
    "dpt_pretok_write": (I32, [P, P, P, U64, P, P, P, P, P]),
    "dpt_pretok_write_atoms": (I32, [P, P, P, U64, P, P, P, P, P]),
    "dpt_debug_pretok_table": (I32, [P, P, U32, P, U32, P, P, U32, I32, P, U64, PU64]),
    # byte-level (BLOOM) pre-tokenization on the device
    "dpt_bytelevel_create": (I32, [P, U32, I32, PP]),
    "dpt_bytelevel_destroy": (I32, [P]),
    "dpt_bytelevel_sizes": (I32, [P, P, P, U64, P, P, P]),
    "dpt_bytelevel_write": (I32, [P, P, P, U64, P, P, P, P, P]),
    "dpt_debug_bytelevel_table": (I32, [P, U32, I32, P, U64, PU64]),
    # the tokenizer's own (greedy BPE) encoding on the device
    "dpt_bpe_create": (I32, [P, P, P, P, U64, I32, PP]),
    "dpt_bpe_destroy": (I32, [P]),
    "dpt_bpe_encode": (I32, [P, P, P, U64, P, P, U64, P, U64, P, P, P, P]),
    "dpt_debug_bpe_lookup": (I32, [P, P, P, P, U64, P, P, U64, P, P]),
    # the two tokenizations compared word by word
    "dpt_word_compare_sizes": (I32, [ctypes.POINTER(WordSide), ctypes.POINTER(WordSide), U64, I32, P, P, P, P, P, P]),
    "dpt_word_compare_write": (I32, [ctypes.POINTER(WordSide), ctypes.POINTER(WordSide), U64, I32] + [P] * 14),
    # sequence packing of an encoded batch into fixed rows
    "dpt_pack_sizes": (I32, [P, P, P, U64, ctypes.POINTER(CollateOpts), P, P]),
    "dpt_pack_plan_workspace": (I32, [U64, PU64]),
    "dpt_pack_plan": (I32, [P, U64, U32, U64, P, P, P, P, P, P, U64, P]),
    "dpt_pack_write": (I32, [ctypes.POINTER(CollateSide), U64, P, P, P, U64, ctypes.POINTER(CollateOpts), P, P, P, P, P]),
    "dpt_debug_pack_geometry": (I32, [ctypes.POINTER(U32), ctypes.POINTER(U32)]),
}
# These came within ABI 6: a libdpt.so from before them (DPT_LIB) lacks the symbols and still encodes;
# ``Detok`` then raises (has_decode).
OPTIONAL = {"dpt_debug_host_layout", "dpt_detok_create", "dpt_detok_destroy", "dpt_decode_sizes", "dpt_decode",
            "dpt_roundtrip", "dpt_decode_host", "dpt_roundtrip_host", "dpt_debug_detok_table"}
EXPORTED = sorted(CALLS)
# the decode calls: name -> argument types
DECODE_CALLS = {name: CALLS[name][1] for name in CALLS if name in OPTIONAL and name != "dpt_debug_host_layout"}
# Also within ABI 6 and probed for like OPTIONAL's (a set of its own: OPTIONAL less the layout call is, by
# tests/test_pack.py, exactly the decode calls); ``collate.collate_device`` raises without it (has_collate),
# ``collate.collate_pair_device`` without dpt_collate_pair (has_collate_pair).
# dpt_debug_wave_grid is test-only: ``wave_grid`` below raises without it.
OPTIONAL_LATER = {"dpt_collate", "dpt_collate_pair", "dpt_debug_wave_grid"}
# Likewise the pre-tokenization calls: name -> argument types; ``pretok.Pretok`` raises without them (has_pretok).
PRETOK_CALLS = {name: CALLS[name][1] for name in CALLS if "_pretok_" in name and name != "dpt_pretok_write_atoms"}
OPTIONAL_PRETOK = set(PRETOK_CALLS)
# And the byte-level split calls; ``bytelevel.ByteLevelSplit`` raises without them (has_bytelevel).
BYTELEVEL_CALLS = {name: CALLS[name][1] for name in CALLS if "_bytelevel_" in name}
OPTIONAL_BYTELEVEL = set(BYTELEVEL_CALLS)
# And the BPE calls, with the pre-tokenization call that makes their llama input; ``bpe.Bpe`` raises without them (has_bpe).
BPE_CALLS = {name: CALLS[name][1] for name in CALLS if "_bpe_" in name or name == "dpt_pretok_write_atoms"}
OPTIONAL_BPE = set(BPE_CALLS)
# And the word-compare calls; ``words.compare_device`` raises without them (has_words).
WORDS_CALLS = {name: CALLS[name][1] for name in CALLS if "_word_compare_" in name}
OPTIONAL_WORDS = set(WORDS_CALLS)
# And the packing calls; ``packing.*_device`` raise without them (has_packing).
PACKING_CALLS = {name: CALLS[name][1] for name in CALLS if "_pack_" in name}
OPTIONAL_PACKING = set(PACKING_CALLS)


def lib():
    """Load libdpt.so (raises DptError when the HIP extension is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("DPT_NO_TORCH", "0") != "1":
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7. Loading it
        # first makes libdpt.so bind to that copy (same SONAME) instead of /opt/rocm's, so device
        # pointers and streams from torch are valid for the engine.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise DptError(f"HIP extension not built: {LIB_PATH} missing (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in CALLS.items():
        if name in OPTIONAL | OPTIONAL_LATER | OPTIONAL_PRETOK | OPTIONAL_BYTELEVEL | OPTIONAL_BPE | OPTIONAL_WORDS | OPTIONAL_PACKING and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def has_decode() -> bool:
    """The loaded library exports the decode calls (a libdpt.so built before them does not)."""
    L = lib()
    return all(hasattr(L, name) for name in DECODE_CALLS)


def has_collate() -> bool:
    """The loaded library exports dpt_collate."""
    return hasattr(lib(), "dpt_collate")


def has_collate_pair() -> bool:
    """The loaded library exports dpt_collate_pair."""
    return hasattr(lib(), "dpt_collate_pair")


def has_pretok() -> bool:
    """The loaded library exports the pre-tokenization calls."""
    L = lib()
    return all(hasattr(L, name) for name in PRETOK_CALLS)


def has_bytelevel() -> bool:
    """The loaded library exports the byte-level split calls."""
    L = lib()
    return all(hasattr(L, name) for name in BYTELEVEL_CALLS)


def has_bpe() -> bool:
    """The loaded library exports the BPE calls."""
    L = lib()
    return all(hasattr(L, name) for name in BPE_CALLS)


def has_words() -> bool:
    """The loaded library exports the word-compare calls."""
    L = lib()
    return all(hasattr(L, name) for name in WORDS_CALLS)


def has_packing() -> bool:
    """The loaded library exports the packing calls."""
    L = lib()
    return all(hasattr(L, name) for name in PACKING_CALLS)


def wave_grid(n_str: int, waves: int = 4) -> int:
    """dpt_debug_wave_grid: the blocks a one-wave-per-string kernel gets for ``n_str`` strings under the current
    environment (DPT_WAVE_GRID_BLOCKS caps it; test-only, needs no device)."""
    L = lib()
    if not hasattr(L, "dpt_debug_wave_grid"):
        raise DptError(f"{LIB_PATH} was built before dpt_debug_wave_grid: rebuild it")
    blocks = U32()
    check(L.dpt_debug_wave_grid(n_str, waves, ctypes.byref(blocks)), "dpt_debug_wave_grid")
    return blocks.value


def check(rc: int, what: str = "") -> None:
    if rc != DPT_OK:
        msg = lib().dpt_last_error().decode("utf-8", "replace")
        raise DptError(f"{what} failed ({rc}): {msg}")


def new_handle(call: str, *args) -> ctypes.c_void_p:
    """A handle from the create call ``call``, whose last argument is the handle out."""
    h = ctypes.c_void_p()
    check(getattr(lib(), call)(*args, ctypes.byref(h)), call)
    return h


def destroy_handle(obj, attr: str, call: str) -> None:
    """Give the handle ``obj.attr`` back through ``call`` if the library is still loaded."""
    h = getattr(obj, attr, None)
    if h and _lib is not None:
        getattr(_lib, call)(h)
        setattr(obj, attr, None)
