"""ctypes binding of libpolars_strsim_amd.so (C ABI: include/strsim_amd.h).

The library is built in-tree by polars-strsim_amd/Makefile into the drop-in package directory
polars_strsim/ (where Polars looks for the plugin).  There is no Python or CPU fallback: if the
library is missing this module raises.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# STRSIM_AMD_LIB: another build of the same library (A/B runs of compile-time variants on one box)
LIB_PATH = os.environ.get("STRSIM_AMD_LIB") or os.path.join(PKG_DIR, "polars_strsim", "libpolars_strsim_amd.so")

MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")  # strsim.rs:9-15
# Measures beyond the reference's five (pairwise entry points only): optimal string alignment = STRSIM_OSA = 6.  MEASURES stays the
# reference's five, the list smoke() and the oracle helpers enumerate.
EXTRA_MEASURES = ("osa",)
MEASURE_ID = {m: i for i, m in enumerate(MEASURES)}
MEASURE_ID["osa"] = 6
# Indel (LCS) similarity = STRSIM_INDEL = 8 (7 stays unassigned): pairwise entry points and the distance calls.  A tuple of its own:
# EXTRA_MEASURES and DISTANCE_MEASURES keep what they listed (nearest() takes DISTANCE_MEASURES, and has no Indel form).
INDEL_MEASURES = ("indel",)
MEASURE_ID["indel"] = 8
# Partial ratio = STRSIM_PARTIAL_RATIO = 10 (9 stays unassigned): pairwise entry points and strsim_partial_alignment_*.  A tuple of
# its own again: it has no distance, no best match, no nearest match and no codec.
PARTIAL_MEASURES = ("partial_ratio",)
MEASURE_ID["partial_ratio"] = 10
# token_sort_ratio = STRSIM_TOKEN_SORT_RATIO = 14, token_set_ratio = STRSIM_TOKEN_SET_RATIO = 16 (11 .. 13 and 15 stay unassigned):
# pairwise entry points only, plus strsim_token_sort_* for the transform itself.  No distance, best match, nearest match or codec.
TOKEN_MEASURES = ("token_sort_ratio", "token_set_ratio")
MEASURE_ID["token_sort_ratio"] = 14
MEASURE_ID["token_set_ratio"] = 16
# token_ratio = 18, partial_token_sort_ratio = 20, partial_token_set_ratio = 22, partial_token_ratio = 24, wratio = STRSIM_WRATIO = 26
# (the odd ids in between stay unassigned): compositions of the measures above, pairwise entry points only.  wratio is rapidfuzz's
# WRatio / 100; the library classifies the rows on the device and runs each family of sub-scores over its own rows.
WEIGHTED_MEASURES = ("token_ratio", "partial_token_sort_ratio", "partial_token_set_ratio", "partial_token_ratio", "wratio")
for _i, _m in enumerate(WEIGHTED_MEASURES):
    MEASURE_ID[_m] = 18 + 2 * _i
ENTRY_POINT_ID = {"pairwise": 0, "best_match": 1, "codec": 2}  # strsim_entry_point_t
# Processors of the processed-scoring calls (strsim_pairs_processed_*): "default_process" = STRSIM_PROCESS_DEFAULT = 1, rapidfuzz's
# utils.default_process made context-free.  None is "no processor".
PROCESSORS = ("default_process",)
PROCESSOR_ID = {"default_process": 1}


def processor_id(processor):
    """The id of a processor name; ValueError for anything that is not one (None, "no processor", is the caller's to handle)."""
    if not isinstance(processor, str) or processor not in PROCESSOR_ID:
        raise ValueError(f"unknown processor {processor!r} (None or one of {PROCESSORS})")
    return PROCESSOR_ID[processor]
# The measures strsim_distance_device / _host accept (integer edit distances), with their ids; STRSIM_DISTANCE_UNBOUNDED = no cutoff.
DISTANCE_MEASURES = ("levenshtein", "osa")
DISTANCE_UNBOUNDED = 0xFFFFFFFF
JOIN_UPPER = 1  # STRSIM_JOIN_UPPER: only pairs with j > i
# The kinds of the q-gram calls (strsim_qgram_device / _host) in the order of their ids, STRSIM_QGRAM_JACCARD = 0 .. _COSINE = 3.  They
# are not measures: q (1 .. QGRAM_MAX_Q) and the mode (STRSIM_QGRAM_SET = 1: sets of grams instead of multisets) come with the call.
QGRAM_KINDS = ("jaccard", "sorensen_dice", "overlap", "cosine")
QGRAM_MAX_Q = 3
QGRAM_SET = 1


# The kinds of strsim_distance_join_* and strsim_distance_cluster_* (STRSIM_EDIT_*), in the order of their ids.
EDIT_KINDS = ("levenshtein", "osa", "damerau_levenshtein")


def edit_kind_id(kind):
    """STRSIM_EDIT_* of a kind; ValueError for one that is not in EDIT_KINDS."""
    if not isinstance(kind, str) or kind not in EDIT_KINDS:
        raise ValueError(f"unknown edit distance {kind!r} (one of {EDIT_KINDS})")
    return EDIT_KINDS.index(kind)


# The kinds of strsim_common_* (STRSIM_COMMON_*), in the order of their ids.
COMMON_KINDS = ("hamming", "prefix", "postfix", "lcs_seq")


def common_kind_id(kind):
    """STRSIM_COMMON_* of a kind; ValueError for one that is not in COMMON_KINDS."""
    if not isinstance(kind, str) or kind not in COMMON_KINDS:
        raise ValueError(f"unknown kind {kind!r} (one of {COMMON_KINDS})")
    return COMMON_KINDS.index(kind)


def qgram_args(kind, q, multiset=True):
    """(kind id, q, flags) of a q-gram call; ValueError for a kind that is not one of QGRAM_KINDS or a q outside 1 .. QGRAM_MAX_Q."""
    if not isinstance(kind, str) or kind not in QGRAM_KINDS:
        raise ValueError(f"unknown q-gram kind {kind!r} (one of {QGRAM_KINDS})")
    if isinstance(q, bool) or not isinstance(q, int) or not 1 <= q <= QGRAM_MAX_Q:
        raise ValueError(f"q={q!r} is outside 1 .. {QGRAM_MAX_Q}")
    return QGRAM_KINDS.index(kind), q, 0 if multiset else QGRAM_SET

STATUS = {0: "OK", 1: "ERR_SHAPE", 2: "ERR_ARG", 3: "ERR_NO_DEVICE", 4: "ERR_HIP", 5: "ERR_OOM", 6: "ERR_DTYPE",
          7: "ERR_INTERNAL", 8: "ERR_EARLIER_CALL"}


class StrsimError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{STATUS.get(code, code)}: {message}")
        self.code = code
        self.message = message


class ShapeMismatch(StrsimError, ValueError):
    """reference: PolarsError::ShapeMismatch, strsim.rs:48-52"""


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.

    torch wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, needed by libtorch_hip.so as plain
    "libamdhip64.so").  Loaded first, this library binds /opt/rocm's copy; a later `import torch` then maps the bundled
    copy NEXT to it (its DT_NEEDED name matches neither the path nor the SONAME of the one already there), and the second
    runtime to initialise reports "No HIP GPUs are available".  Mapping torch's copy before ours makes the loader resolve
    our DT_NEEDED libamdhip64.so.7 by SONAME to it, and torch finds the same file already mapped.  A process without
    torch (the Polars plugin route) is not affected and runs on /opt/rocm's runtime.
    """
    import sys
    if "torch" in sys.modules or os.environ.get("STRSIM_KEEP_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` (hipcc, gfx950). "
            "polars-strsim_amd has no Python/CPU fallback.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.strsim_abi_version.restype = C.c_uint32
    L.strsim_abi_version.argtypes = []
    L.strsim_last_error_message.restype = C.c_char_p
    L.strsim_last_error_message.argtypes = []
    L.strsim_device_count.restype = i32
    L.strsim_device_count.argtypes = []
    L.strsim_ctx_create.restype = i32
    L.strsim_ctx_create.argtypes = [i32, vp, C.POINTER(vp)]
    L.strsim_ctx_destroy.restype = None
    L.strsim_ctx_destroy.argtypes = [vp]
    L.strsim_ctx_stream.restype = vp
    L.strsim_ctx_stream.argtypes = [vp]
    for name in ("strsim_pairs_device", "strsim_pairs_device_small", "strsim_pairs_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_best_match_device", "strsim_best_match_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_double, vp, vp]
    for name in ("strsim_distance_device", "strsim_distance_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, vp, u64]
    for name in ("strsim_qgram_device", "strsim_qgram_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, C.c_uint32, C.c_uint32, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_damerau_device", "strsim_damerau_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_damerau_distance_device", "strsim_damerau_distance_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.c_uint32, vp, u64]
    for name in ("strsim_common_device", "strsim_common_host", "strsim_common_count_device", "strsim_common_count_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, vp, u64]
    for name in ("strsim_common_distance_device", "strsim_common_distance_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, vp, u64]
    for name in ("strsim_partial_alignment_device", "strsim_partial_alignment_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_token_sort_device", "strsim_token_sort_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64]
    L.strsim_ctx_last_token_wave_rows.restype = u64
    L.strsim_ctx_last_token_wave_rows.argtypes = [vp]
    for name in ("strsim_default_process_device", "strsim_default_process_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, vp, vp, u64, vp, vp, u64]
    for name in ("strsim_pairs_processed_device", "strsim_pairs_processed_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, i32, vp, vp, u64, vp, vp, u64, vp, u64]
    L.strsim_ctx_last_process_wave_rows.restype = u64
    L.strsim_ctx_last_process_wave_rows.argtypes = [vp]
    L.strsim_default_process_char.restype = C.c_uint32
    L.strsim_default_process_char.argtypes = [C.c_uint32]
    L.strsim_default_process_unicode_version.restype = C.c_char_p
    L.strsim_default_process_unicode_version.argtypes = []
    L.strsim_ctx_last_wratio_rows.restype = i32
    L.strsim_ctx_last_wratio_rows.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    for name in ("strsim_nearest_device", "strsim_nearest_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp]
    for name in ("strsim_extract_device", "strsim_extract_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_double, vp, vp]
    for name in ("strsim_cdist_device", "strsim_cdist_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_double, vp, u64]
    for name in ("strsim_join_device", "strsim_join_host", "strsim_match_join_device", "strsim_match_join_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_double, C.c_uint32, u64, vp, vp, vp, C.POINTER(u64)]
    for name in ("strsim_qgram_join_device", "strsim_qgram_join_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, C.c_uint32, C.c_uint32, vp, vp, u64, vp, vp, u64, C.c_double, C.c_uint32, u64, vp, vp, vp, C.POINTER(u64)]
    for name in ("strsim_qgram_cluster_device", "strsim_qgram_cluster_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, C.c_uint32, C.c_uint32, vp, vp, u64, C.c_double, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    for name in ("strsim_distance_join_device", "strsim_distance_join_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, C.c_uint32, C.c_uint32, u64, vp, vp, vp, C.POINTER(u64)]
    for name in ("strsim_distance_cluster_device", "strsim_distance_cluster_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, C.c_uint32, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    for name in ("strsim_components_device", "strsim_components_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, u64, vp, vp, u64, vp, vp, C.POINTER(u64)]
    for name in ("strsim_cluster_device", "strsim_cluster_host"):
        f = getattr(L, name)
        f.restype = i32
        f.argtypes = [vp, i32, vp, vp, u64, C.c_double, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.strsim_measure_supported.restype = C.c_uint32
    L.strsim_measure_supported.argtypes = [i32, i32]
    L.strsim_pairs_device_all.restype = i32
    L.strsim_pairs_device_all.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(vp), u64]
    L.strsim_codec_create.restype = i32
    L.strsim_codec_create.argtypes = [vp, i32, C.c_uint32, C.POINTER(vp)]
    L.strsim_codec_destroy.restype = None
    L.strsim_codec_destroy.argtypes = [vp]
    L.strsim_codec_entries.restype = C.c_uint32
    L.strsim_codec_entries.argtypes = [vp]
    L.strsim_codec_encode.restype = i32
    L.strsim_codec_encode.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, C.c_uint32]
    L.strsim_codec_decode.restype = i32
    L.strsim_codec_decode.argtypes = [vp, vp, vp, u64, vp]
    L.strsim_codec_bits.restype = C.c_uint32
    L.strsim_codec_bits.argtypes = [vp]
    L.strsim_codec_packed_words.restype = u64
    L.strsim_codec_packed_words.argtypes = [vp, u64]
    L.strsim_codec_encode_packed.restype = i32
    L.strsim_codec_encode_packed.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, C.c_uint32]
    L.strsim_codec_decode_packed.restype = i32
    L.strsim_codec_decode_packed.argtypes = [vp, vp, vp, u64, vp]
    L.strsim_codec_patch.restype = i32
    L.strsim_codec_patch.argtypes = [vp, vp, u64, vp, vp, C.c_uint32]
    L.strsim_offsets_from_lengths.restype = i32
    L.strsim_offsets_from_lengths.argtypes = [vp, vp, u64, vp]
    L.strsim_ctx_retire_oldest.restype = i32
    L.strsim_ctx_retire_oldest.argtypes = [vp]
    L.strsim_codec_patch_indirect.restype = i32
    L.strsim_codec_patch_indirect.argtypes = [vp, vp, u64, vp, vp, vp, C.c_uint32, vp]
    L.strsim_ctx_synchronize.restype = i32
    L.strsim_ctx_synchronize.argtypes = [vp]
    L.strsim_split_offsets.restype = None
    L.strsim_split_offsets.argtypes = [u64, u64, vp]
    L.strsim_ctx_timing_enable.restype = i32
    L.strsim_ctx_timing_enable.argtypes = [vp, i32]
    L.strsim_ctx_timing_read.restype = i32
    L.strsim_ctx_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(C.c_double),
                                         C.POINTER(u64)]
    L.strsim_ctx_last_wave_rows.restype = u64
    L.strsim_ctx_last_wave_rows.argtypes = [vp]
    L.strsim_ctx_last_long_rows.restype = u64
    L.strsim_ctx_last_long_rows.argtypes = [vp]
    L.strsim_column_from_views.restype = i32
    L.strsim_column_from_views.argtypes = [vp, vp, u64, vp, vp, vp]
    L.strsim_column_from_views_bounded.restype = i32
    L.strsim_column_from_views_bounded.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp]
    L.strsim_ctx_last_late_rows.restype = u64
    L.strsim_ctx_last_late_rows.argtypes = [vp]
    L.strsim_codec_decode_gathered.restype = i32
    L.strsim_codec_decode_gathered.argtypes = [vp, vp, vp, u64, C.c_uint32, u64, u64, i32, u64, C.c_uint32, vp, vp]
    L.strsim_gather_unique_id.restype = i32
    L.strsim_gather_unique_id.argtypes = [vp]
    L.strsim_gather_create.restype = i32
    L.strsim_gather_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.strsim_gather_f64.restype = i32
    L.strsim_gather_f64.argtypes = [vp, vp, vp, u64, i32]
    L.strsim_ctx_get_stream_ordered.restype = i32
    L.strsim_ctx_get_stream_ordered.argtypes = [vp]
    L.strsim_gather_f64_ranges.restype = i32
    L.strsim_gather_f64_ranges.argtypes = [vp, vp, vp, vp, i32]
    L.strsim_gather_comm_count.restype = i32
    L.strsim_gather_comm_count.argtypes = [vp, C.POINTER(i32)]
    L.strsim_gather_destroy.restype = None
    L.strsim_gather_destroy.argtypes = [vp]
    L.strsim_codec_decode_gathered_from.restype = i32
    L.strsim_codec_decode_gathered_from.argtypes = [vp, vp, vp, u64, C.c_uint32, C.c_uint32, u64, u64, i32, u64, C.c_uint32, vp, vp]
    L.strsim_compact_segments.restype = i32
    L.strsim_compact_segments.argtypes = [vp, vp, vp, vp, vp, vp, i32]
    L.strsim_ctx_enqueued_ops.restype = u64
    L.strsim_ctx_enqueued_ops.argtypes = [vp]
    L.strsim_ctx_set_stream_ordered.restype = i32
    L.strsim_ctx_set_stream_ordered.argtypes = [vp, i32]
    _lib = L
    return L


def check(rc):
    if rc == 0:
        return
    msg = lib().strsim_last_error_message().decode("utf-8", "replace")
    if rc == 1:
        raise ShapeMismatch(rc, msg)
    raise StrsimError(rc, msg)


def measure_id(measure):
    if isinstance(measure, str):
        return MEASURE_ID[measure]
    return int(measure)
