"""Device context + the two compute entry points of the C ABI, for numpy (host) and torch (device) buffers."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DISTANCE_UNBOUNDED, JOIN_UPPER, StrsimError, check, common_kind_id, edit_kind_id, lib, measure_id, processor_id, qgram_args


def split_offsets(length, n):
    """Row partition of the reference's split_offsets (strsim.rs:21-39) -> [(offset, len)] * n."""
    out = np.zeros(2 * n, dtype=np.uint64)
    lib().strsim_split_offsets(int(length), int(n), out.ctypes.data)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def device_count():
    return int(lib().strsim_device_count())


class Context:
    """One GPU + one HIP stream + workspace (include/strsim_amd.h: strsim_ctx_t).  One per thread."""

    def __init__(self, device=0, stream=None, one_launch=False):
        """`one_launch`: opt in to one-launch calls (strsim_ctx_set_stream_ordered(ctx, 0), ABI 1.4): a call that is expected to
        need the first kernel only is enqueued as that kernel alone, and slow rows it turns out to hold are finished when the
        call is retired -- for callers that synchronize() / retire_oldest() before they read results.  Default: every row of
        strings <= 1024 bytes is complete in stream order.
        `stream`: an int hipStream_t (e.g. torch.cuda.Stream().cuda_stream), or None for an own non-blocking stream.
        Handle 0 -- torch's DEFAULT stream, `torch.cuda.current_stream().cuda_stream` outside a `torch.cuda.stream(s)`
        block -- is refused: the C ABI reads NULL as "create your own stream", so the context would silently run on a
        stream that torch-side events and copies are not ordered against.  Pass a real torch stream and do the torch-side
        work (event.record(s), .cpu()) under `torch.cuda.stream(s)`, or pass None and use ctx.synchronize()."""
        if stream is not None and int(stream) == 0:
            raise ValueError("stream handle 0 is the default stream: pass None for an own stream, or a torch.cuda.Stream()'s "
                             "cuda_stream (and run the torch-side work under torch.cuda.stream(s))")
        self._h = C.c_void_p()
        check(lib().strsim_ctx_create(int(device), C.c_void_p(int(stream)) if stream is not None else None, C.byref(self._h)))
        self.device = int(device)
        if one_launch:
            self.set_stream_ordered(False)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().strsim_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def stream(self):
        return lib().strsim_ctx_stream(self._h)

    def synchronize(self):
        check(lib().strsim_ctx_synchronize(self._h))

    def timing(self, enable=True):
        check(lib().strsim_ctx_timing_enable(self._h, 1 if enable else 0))

    def timing_read(self):
        """-> dict(lane_ms, lane_launches, wave_ms, wave_launches) accumulated since the last read."""
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_uint64(), C.c_uint64()
        check(lib().strsim_ctx_timing_read(self._h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return {"lane_ms": a.value, "lane_launches": na.value, "wave_ms": b.value, "wave_launches": nb.value}

    @property
    def last_wave_rows(self):
        return int(lib().strsim_ctx_last_wave_rows(self._h))

    @property
    def last_token_wave_rows(self):
        """Rows the last token call (token_sort_*, or a pairwise call of token_sort_ratio / token_set_ratio) rewrote one string per
        wave, both columns added up; 0 when every row took the one-string-per-lane tier.  Valid once the stream has completed
        that call (synchronize())."""
        return int(lib().strsim_ctx_last_token_wave_rows(self._h))

    @property
    def last_process_wave_rows(self):
        """Rows the last default_process_* / pairs_processed_* call rewrote one string per wave (non-ASCII, or longer than 64 bytes),
        both columns added up; 0 when every row took the one-string-per-lane tier.  Valid when that call has returned."""
        return int(lib().strsim_ctx_last_process_wave_rows(self._h))

    def last_wratio_rows(self):
        """-> (near, far): how the last completed wratio call routed its rows -- to the token family (2 hi < 3 lo in characters)
        or to the partial family; rows in neither count had an empty string."""
        near, far = C.c_uint64(), C.c_uint64()
        check(lib().strsim_ctx_last_wratio_rows(self._h, C.byref(near), C.byref(far)))
        return int(near.value), int(far.value)

    @property
    def last_late_rows(self):
        """Rows finished by a pass that the last synchronize() / retire_oldest() launched (slow rows of a one-launch call,
        long strings): written AFTER whatever was enqueued on the stream behind the call."""
        return int(lib().strsim_ctx_last_late_rows(self._h))

    @property
    def enqueued_ops(self):
        """Kernels + device copies enqueued for pair calls so far (1 per call when no slow rows are expected, else 5)."""
        return int(lib().strsim_ctx_enqueued_ops(self._h))

    def set_stream_ordered(self, enable=True):
        """True (the default of a new context): every call enqueues all its kernels up front, so results (strings <= 1024
        bytes) are complete in stream order -- for callers that consume them behind an event without retiring the call.
        False: one-launch calls (see __init__).  Takes effect with the next call (strsim_ctx_set_stream_ordered)."""
        check(lib().strsim_ctx_set_stream_ordered(self._h, 1 if enable else 0))

    @property
    def stream_ordered(self):
        """The mode the next call is enqueued in (strsim_ctx_get_stream_ordered, ABI 1.6): True = every kernel up front."""
        return bool(lib().strsim_ctx_get_stream_ordered(self._h))

    @property
    def last_long_rows(self):
        """Rows with a string beyond the wave-kernel cap among the calls the last synchronize() retired."""
        return int(lib().strsim_ctx_last_long_rows(self._h))

    # ---- device-resident (torch tensors on this context's GPU) -------------------------------------
    def pairs_device(self, measure, a_offsets, a_values, b_offsets, b_values, out=None):
        """Enqueue one pass; tensors are torch CUDA tensors (offsets int32/uint32 [rows+1], values uint8).
        Returns the f64 output tensor; complete after synchronize()."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.float64, device=a_offsets.device)
        check(lib().strsim_pairs_device(self._h, measure_id(measure),
                                        a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                        b_offsets.data_ptr(), b_values.data_ptr(), rb,
                                        out.data_ptr(), out.numel()))
        return out

    def offsets_from_lengths(self, lengths, out=None):
        """uint8 device tensor of string lengths -> uint32 offsets (rows + 1) on the device (strsim_offsets_from_lengths)."""
        import torch
        n = lengths.numel()
        if out is None:
            out = torch.empty(n + 1, dtype=torch.int32, device=lengths.device)
        check(lib().strsim_offsets_from_lengths(self._h, lengths.data_ptr(), int(n), out.data_ptr()))
        return out

    def column_from_views(self, views, long_values, packed_bytes, bounded=True):
        """Utf8View slots on the device (uint8 tensor of rows x 16 bytes; slots of strings beyond 12 bytes carry their offset in
        `long_values` in their last word) -> (offsets int32 [rows + 1], values uint8 [packed_bytes + 64]).  `bounded` (ABI 1.5,
        strsim_column_from_views_bounded): the extents of both buffers are stated, a slot that reaches outside them is skipped and
        counted -> a third result, an int32 tensor of one element (read it after synchronize()); False: strsim_column_from_views."""
        import torch
        rows = views.numel() // 16
        off = torch.empty(rows + 1, dtype=torch.int32, device=views.device)
        val = torch.zeros(int(packed_bytes) + 64, dtype=torch.uint8, device=views.device)
        if not bounded:
            check(lib().strsim_column_from_views(self._h, views.data_ptr(), rows, long_values.data_ptr() if long_values is not None else None,
                                                 off.data_ptr(), val.data_ptr()))
            return off, val
        bad = torch.zeros(1, dtype=torch.int32, device=views.device)
        check(lib().strsim_column_from_views_bounded(self._h, views.data_ptr(), rows,
                                                     long_values.data_ptr() if long_values is not None else None,
                                                     long_values.numel() if long_values is not None else 0,
                                                     off.data_ptr(), val.data_ptr(), val.numel(), bad.data_ptr()))
        return off, val, bad

    def retire_oldest(self):
        """Retire the oldest pending call only (the caller knows by an event of its own that it has completed)."""
        check(lib().strsim_ctx_retire_oldest(self._h))

    def pairs_device_all(self, a_offsets, a_values, b_offsets, b_values, outs=None):
        """All five measures in one fused call -> list of five f64 tensors indexed like MEASURES."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        if outs is None:
            outs = [torch.empty(n, dtype=torch.float64, device=a_offsets.device) for _ in range(5)]
        arr = (C.c_void_p * 5)(*[o.data_ptr() for o in outs])
        check(lib().strsim_pairs_device_all(self._h, a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                            b_offsets.data_ptr(), b_values.data_ptr(), rb, arr, n))
        return outs

    def distance_device(self, measure, a_offsets, a_values, b_offsets, b_values, max_distance=None, out=None):
        """Bounded edit distances (strsim_distance_device) of device tensors laid out as for pairs_device -> uint32 values in an
        int32 tensor (torch has no uint32 arithmetic; read it with .view or & 0xFFFFFFFF).  measure: "levenshtein" or "osa";
        max_distance=None is no cutoff, else rows beyond it hold max_distance + 1.  Complete in stream order."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.int32, device=a_offsets.device)
        assert out.is_cuda and out.device == a_offsets.device and out.element_size() == 4 and out.is_contiguous() \
            and not out.is_floating_point(), "out must be a contiguous 4-byte integer tensor on the inputs' device"
        check(lib().strsim_distance_device(self._h, measure_id(measure), a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                           b_offsets.data_ptr(), b_values.data_ptr(), rb, _max_distance(max_distance),
                                           out.data_ptr(), out.numel()))
        return out

    def qgram_device(self, kind, a_offsets, a_values, b_offsets, b_values, q=2, multiset=True, out=None):
        """q-gram similarity (strsim_qgram_device) of device tensors laid out as for pairs_device -> f64 tensor.  kind: one of
        QGRAM_KINDS; q: 1, 2 or 3; multiset=False compares the sets of grams.  Complete in stream order; last_wave_rows counts the
        rows that took the one-pair-per-wave tier."""
        import torch
        kid, q, flags = qgram_args(kind, q, multiset)
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.float64, device=a_offsets.device)
        check(lib().strsim_qgram_device(self._h, kid, q, flags, a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                        b_offsets.data_ptr(), b_values.data_ptr(), rb, out.data_ptr(), out.numel()))
        return out

    def damerau_device(self, a_offsets, a_values, b_offsets, b_values, out=None):
        """Unrestricted Damerau-Levenshtein similarity (strsim_damerau_device) of device tensors laid out as for pairs_device -> f64
        tensor.  Complete in stream order; last_wave_rows counts the rows that took the one-pair-per-wave tier."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.float64, device=a_offsets.device)
        check(lib().strsim_damerau_device(self._h, a_offsets.data_ptr(), a_values.data_ptr(), ra, b_offsets.data_ptr(), b_values.data_ptr(),
                                          rb, out.data_ptr(), out.numel()))
        return out

    def damerau_distance_device(self, a_offsets, a_values, b_offsets, b_values, max_distance=None, out=None):
        """Unrestricted Damerau-Levenshtein distance (strsim_damerau_distance_device) of device tensors -> uint32 values in an int32
        tensor, as distance_device returns them.  max_distance=None is no cutoff, else rows beyond it hold max_distance + 1."""
        import torch
        k = _max_distance(max_distance)
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.int32, device=a_offsets.device)
        assert out.is_cuda and out.device == a_offsets.device and out.element_size() == 4 and out.is_contiguous() \
            and not out.is_floating_point(), "out must be a contiguous 4-byte integer tensor on the inputs' device"
        check(lib().strsim_damerau_distance_device(self._h, a_offsets.data_ptr(), a_values.data_ptr(), ra, b_offsets.data_ptr(),
                                                   b_values.data_ptr(), rb, k, out.data_ptr(), out.numel()))
        return out

    def _common_device(self, call, kind, a_offsets, a_values, b_offsets, b_values, out, dtype, *extra):
        import torch
        kid = common_kind_id(kind)
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=dtype, device=a_offsets.device)
        if dtype != torch.float64:
            assert out.is_cuda and out.device == a_offsets.device and out.element_size() == 4 and out.is_contiguous() \
                and not out.is_floating_point(), "out must be a contiguous 4-byte integer tensor on the inputs' device"
        check(call(self._h, kid, a_offsets.data_ptr(), a_values.data_ptr(), ra, b_offsets.data_ptr(), b_values.data_ptr(), rb, *extra,
                   out.data_ptr(), out.numel()))
        return out

    def common_device(self, kind, a_offsets, a_values, b_offsets, b_values, out=None):
        """Normalised similarity of a COMMON_KINDS kind ("hamming", "prefix", "postfix", "lcs_seq"; strsim_common_device) of device
        tensors laid out as for pairs_device -> f64 tensor: 1 - distance / max(len), 1.0 when both are empty.  Complete in stream
        order; last_wave_rows counts the rows that took the one-pair-per-wave tier."""
        import torch
        return self._common_device(lib().strsim_common_device, kind, a_offsets, a_values, b_offsets, b_values, out, torch.float64)

    def common_distance_device(self, kind, a_offsets, a_values, b_offsets, b_values, max_distance=None, out=None):
        """Distance of a COMMON_KINDS kind (strsim_common_distance_device): max(len) - count, uint32 values in an int32 tensor, as
        distance_device returns them.  max_distance=None is no cutoff, else rows beyond it hold max_distance + 1."""
        import torch
        k = _max_distance(max_distance)
        return self._common_device(lib().strsim_common_distance_device, kind, a_offsets, a_values, b_offsets, b_values, out, torch.int32, k)

    def common_count_device(self, kind, a_offsets, a_values, b_offsets, b_values, out=None):
        """Count of common characters of a COMMON_KINDS kind (strsim_common_count_device; rapidfuzz's similarity) -> uint32 values
        in an int32 tensor."""
        import torch
        return self._common_device(lib().strsim_common_count_device, kind, a_offsets, a_values, b_offsets, b_values, out, torch.int32)

    def partial_alignment_device(self, a_offsets, a_values, b_offsets, b_values, score=None, span=None):
        """Partial ratio with its alignment (strsim_partial_alignment_device) of device tensors laid out as for pairs_device ->
        (score f64 [n], span int32 [n, 4] holding uint32 a_start, a_end, b_start, b_end in characters).  Complete in stream order."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        rows = n if (ra == rb or ra == 1 or rb == 1) else 0
        if score is None:
            score = torch.empty(rows, dtype=torch.float64, device=a_offsets.device)
        if span is None:
            span = torch.empty((rows, 4), dtype=torch.int32, device=a_offsets.device)
        assert span.is_cuda and span.element_size() == 4 and span.is_contiguous() and not span.is_floating_point()
        check(lib().strsim_partial_alignment_device(self._h, a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                                    b_offsets.data_ptr(), b_values.data_ptr(), rb,
                                                    score.data_ptr(), span.data_ptr(), score.numel()))
        return score, span

    def token_sort_device(self, offsets, values, out_offsets=None, out_values=None):
        """The token_sort transform (strsim_token_sort_device) of a device column laid out as for pairs_device -> (offsets int32
        [rows + 1], values uint8): row i becomes join(sorted(tokens(row i))).  out_values must hold the input's bytes (the
        default: as many as `values`).  Complete in stream order; the call waits once for the stream at its start."""
        import torch
        rows = offsets.numel() - 1
        _check_device_column(offsets, values)
        if out_offsets is None:
            out_offsets = torch.empty(rows + 1, dtype=torch.int32, device=offsets.device)
        if out_values is None:
            out_values = torch.empty(max(values.numel(), 1), dtype=torch.uint8, device=offsets.device)
        _check_device_column(out_offsets, out_values)
        assert out_offsets.numel() == rows + 1
        check(lib().strsim_token_sort_device(self._h, offsets.data_ptr(), values.data_ptr(), rows, out_offsets.data_ptr(),
                                             out_values.data_ptr(), out_values.numel()))
        return out_offsets, out_values

    def default_process_device(self, offsets, values, out_offsets=None, out_values=None):
        """default_process (strsim_default_process_device) of a device column laid out as for pairs_device -> (offsets int32
        [rows + 1], values uint8): row i is lower-cased, every scalar value that is neither alphanumeric nor "_" becomes a space,
        and spaces are removed from both ends.  A processed row can be longer than its input: out_values defaults to
        bytes + bytes / 2, which always suffices; offsets[rows] is the exact size.  Complete in stream order; the call waits once
        for the stream (between its measuring and its writing pass)."""
        import torch
        rows = offsets.numel() - 1
        _check_device_column(offsets, values)
        if out_offsets is None:
            out_offsets = torch.empty(rows + 1, dtype=torch.int32, device=offsets.device)
        if out_values is None:
            out_values = torch.empty(max(values.numel() + values.numel() // 2, 1), dtype=torch.uint8, device=offsets.device)
        _check_device_column(out_offsets, out_values)
        assert out_offsets.numel() == rows + 1
        check(lib().strsim_default_process_device(self._h, offsets.data_ptr(), values.data_ptr(), rows, out_offsets.data_ptr(),
                                                  out_values.data_ptr(), out_values.numel()))
        return out_offsets, out_values

    def pairs_processed_device(self, measure, a_offsets, a_values, b_offsets, b_values, out=None, processor="default_process"):
        """pairs_device over the processed columns (strsim_pairs_processed_device): both sides go through `processor` on the
        device, into scratch of the context, and `measure` runs over the result -- bit for bit pairs_device(measure) over
        default_process_device of each side.  Returns the f64 output tensor; complete after synchronize()."""
        import torch
        ra, rb = a_offsets.numel() - 1, b_offsets.numel() - 1
        n = rb if ra == 1 else ra
        _check_device_column(a_offsets, a_values)
        _check_device_column(b_offsets, b_values)
        if out is None:
            out = torch.empty(n if (ra == rb or ra == 1 or rb == 1) else 0, dtype=torch.float64, device=a_offsets.device)
        check(lib().strsim_pairs_processed_device(self._h, measure_id(measure), processor_id(processor),
                                                  a_offsets.data_ptr(), a_values.data_ptr(), ra,
                                                  b_offsets.data_ptr(), b_values.data_ptr(), rb,
                                                  out.data_ptr(), out.numel()))
        return out

    # ---- host-resident (numpy) ---------------------------------------------------------------------
    def default_process_host(self, offsets, values):
        """Synchronous default_process (strsim_default_process_host): numpy uint32 offsets + uint8 values in -> (uint32 offsets
        from 0, uint8 values of offsets[-1] bytes)."""
        off, val, rows = _host_column(offsets, values)
        out_off = np.empty(rows + 1, dtype=np.uint32)
        cap = int(off[rows]) - int(off[0])
        cap += cap // 2
        out_val = np.empty(max(cap, 1), dtype=np.uint8)
        check(lib().strsim_default_process_host(self._h, off.ctypes.data, val.ctypes.data, rows, out_off.ctypes.data, out_val.ctypes.data, cap))
        return out_off, out_val[:int(out_off[rows])]

    def pairs_processed_host(self, measure, a_offsets, a_values, b_offsets, b_values, processor="default_process"):
        """Synchronous processed scoring (strsim_pairs_processed_host): numpy uint32 offsets + uint8 values in, numpy f64 out."""
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.float64)
        check(lib().strsim_pairs_processed_host(self._h, measure_id(measure), processor_id(processor), ao.ctypes.data, av.ctypes.data, ra,
                                                bo.ctypes.data, bv.ctypes.data, rb, out.ctypes.data, n))
        return out

    def token_sort_host(self, offsets, values):
        """Synchronous token_sort transform (strsim_token_sort_host): numpy uint32 offsets + uint8 values in -> (uint32 offsets
        from 0, uint8 values of offsets[-1] bytes)."""
        off, val, rows = _host_column(offsets, values)
        out_off = np.empty(rows + 1, dtype=np.uint32)
        cap = int(off[rows]) - int(off[0])
        out_val = np.empty(max(cap, 1), dtype=np.uint8)
        check(lib().strsim_token_sort_host(self._h, off.ctypes.data, val.ctypes.data, rows, out_off.ctypes.data, out_val.ctypes.data, cap))
        return out_off, out_val[:int(out_off[rows])]

    def pairs_host(self, measure, a_offsets, a_values, b_offsets, b_values):
        """Synchronous: numpy uint32 offsets + uint8 values in, numpy f64 out."""
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.float64)
        check(lib().strsim_pairs_host(self._h, measure_id(measure), ao.ctypes.data, av.ctypes.data, ra,
                                      bo.ctypes.data, bv.ctypes.data, rb, out.ctypes.data, n))
        return out

    def distance_host(self, measure, a_offsets, a_values, b_offsets, b_values, max_distance=None):
        """Synchronous bounded edit distances (strsim_distance_host): numpy uint32 offsets + uint8 values in, numpy uint32 out."""
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.uint32)
        check(lib().strsim_distance_host(self._h, measure_id(measure), ao.ctypes.data, av.ctypes.data, ra,
                                         bo.ctypes.data, bv.ctypes.data, rb, _max_distance(max_distance), out.ctypes.data, n))
        return out

    def qgram_host(self, kind, a_offsets, a_values, b_offsets, b_values, q=2, multiset=True):
        """Synchronous q-gram similarity (strsim_qgram_host): numpy uint32 offsets + uint8 values in, numpy f64 out.  kind: one of
        QGRAM_KINDS; q: 1, 2 or 3; multiset=False compares the sets of grams."""
        kid, q, flags = qgram_args(kind, q, multiset)
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.float64)
        check(lib().strsim_qgram_host(self._h, kid, q, flags, ao.ctypes.data, av.ctypes.data, ra, bo.ctypes.data, bv.ctypes.data, rb,
                                      out.ctypes.data, n))
        return out

    def damerau_host(self, a_offsets, a_values, b_offsets, b_values):
        """Synchronous unrestricted Damerau-Levenshtein similarity (strsim_damerau_host): numpy uint32 offsets + uint8 values in,
        numpy f64 out."""
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.float64)
        check(lib().strsim_damerau_host(self._h, ao.ctypes.data, av.ctypes.data, ra, bo.ctypes.data, bv.ctypes.data, rb, out.ctypes.data, n))
        return out

    def damerau_distance_host(self, a_offsets, a_values, b_offsets, b_values, max_distance=None):
        """Synchronous unrestricted Damerau-Levenshtein distance (strsim_damerau_distance_host): numpy uint32 offsets + uint8 values
        in, numpy uint32 out."""
        k = _max_distance(max_distance)
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=np.uint32)
        check(lib().strsim_damerau_distance_host(self._h, ao.ctypes.data, av.ctypes.data, ra, bo.ctypes.data, bv.ctypes.data, rb, k,
                                                 out.ctypes.data, n))
        return out

    def _common_host(self, call, kind, a_offsets, a_values, b_offsets, b_values, dtype, *extra):
        kid = common_kind_id(kind)
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        out = np.empty(n, dtype=dtype)
        check(call(self._h, kid, ao.ctypes.data, av.ctypes.data, ra, bo.ctypes.data, bv.ctypes.data, rb, *extra, out.ctypes.data, n))
        return out

    def common_host(self, kind, a_offsets, a_values, b_offsets, b_values):
        """Synchronous normalised similarity of a COMMON_KINDS kind (strsim_common_host): numpy uint32 offsets + uint8 values in,
        numpy f64 out."""
        return self._common_host(lib().strsim_common_host, kind, a_offsets, a_values, b_offsets, b_values, np.float64)

    def common_distance_host(self, kind, a_offsets, a_values, b_offsets, b_values, max_distance=None):
        """Synchronous distance of a COMMON_KINDS kind (strsim_common_distance_host): numpy uint32 out."""
        k = _max_distance(max_distance)
        return self._common_host(lib().strsim_common_distance_host, kind, a_offsets, a_values, b_offsets, b_values, np.uint32, k)

    def common_count_host(self, kind, a_offsets, a_values, b_offsets, b_values):
        """Synchronous count of common characters of a COMMON_KINDS kind (strsim_common_count_host): numpy uint32 out."""
        return self._common_host(lib().strsim_common_count_host, kind, a_offsets, a_values, b_offsets, b_values, np.uint32)

    def partial_alignment_host(self, a_offsets, a_values, b_offsets, b_values):
        """Synchronous partial ratio with its alignment (strsim_partial_alignment_host): numpy uint32 offsets + uint8 values in ->
        (score f64 [n], span uint32 [n, 4]: a_start, a_end, b_start, b_end, half open, in characters)."""
        ao, av, ra = _host_column(a_offsets, a_values)
        bo, bv, rb = _host_column(b_offsets, b_values)
        n = _rows_out(ra, rb)
        score = np.empty(n, dtype=np.float64)
        span = np.empty((n, 4), dtype=np.uint32)
        check(lib().strsim_partial_alignment_host(self._h, ao.ctypes.data, av.ctypes.data, ra, bo.ctypes.data, bv.ctypes.data, rb,
                                                  score.ctypes.data, span.ctypes.data, n))
        return score, span

    def best_match(self, measure, q_offsets, q_values, c_offsets, c_values, k=1, min_score=None):
        """Synchronous best match (strsim_best_match_host, ABI 1.7): numpy uint32 offsets + uint8 values of the queries and the
        candidates -> (index uint32 [rows, k], score f64 [rows, k]), each query's k best candidates by descending score, ties to the
        lower index; empty slots are (0xFFFFFFFF, NaN).  min_score=None reports every candidate."""
        qo, qv, nq = _host_column(q_offsets, q_values)
        co, cv, nc = _host_column(c_offsets, c_values)
        index = np.empty((nq, int(k)), dtype=np.uint32)
        score = np.empty((nq, int(k)), dtype=np.float64)
        ms = -np.inf if min_score is None else float(min_score)
        check(lib().strsim_best_match_host(self._h, measure_id(measure), qo.ctypes.data, qv.ctypes.data, nq,
                                           co.ctypes.data, cv.ctypes.data, nc, int(k), ms, index.ctypes.data, score.ctypes.data))
        return index, score

    def nearest(self, measure, q_offsets, q_values, c_offsets, c_values, k=1, max_distance=None):
        """Synchronous nearest match (strsim_nearest_host): numpy uint32 offsets + uint8 values of the queries and the candidates ->
        (index uint32 [rows, k], distance uint32 [rows, k]), each query's k nearest candidates by edit distance ("levenshtein" or
        "osa"), ascending, ties to the lower index; only d <= max_distance is reported (None: no cutoff).  Empty slots are
        (0xFFFFFFFF, 0xFFFFFFFF)."""
        qo, qv, nq = _host_column(q_offsets, q_values)
        co, cv, nc = _host_column(c_offsets, c_values)
        index = np.empty((nq, int(k)), dtype=np.uint32)
        dist = np.empty((nq, int(k)), dtype=np.uint32)
        check(lib().strsim_nearest_host(self._h, measure_id(measure), qo.ctypes.data, qv.ctypes.data, nq,
                                        co.ctypes.data, cv.ctypes.data, nc, int(k), _max_distance(max_distance),
                                        index.ctypes.data, dist.ctypes.data))
        return index, dist

    def extract(self, scorer, q_offsets, q_values, c_offsets, c_values, k=1, score_cutoff=None):
        """Top-k search by "indel" (rapidfuzz's ratio / 100) or "token_sort_ratio" (strsim_extract_host for numpy columns,
        strsim_extract_device for torch tensors on this context's device): uint32 offsets + uint8 values of the queries and the
        candidates -> (index uint32 [rows, k], score f64 [rows, k]), each query's k best candidates by descending score, ties to
        the lower index; only scores >= score_cutoff are reported (None: no cutoff).  Empty slots are (0xFFFFFFFF, NaN).  Device
        inputs give device outputs, complete in stream order."""
        cut = -np.inf if score_cutoff is None else float(score_cutoff)
        if not isinstance(q_offsets, np.ndarray) and hasattr(q_offsets, "data_ptr"):
            import torch
            nq, nc = q_offsets.numel() - 1, max(c_offsets.numel() - 1, 0)
            index = torch.empty((nq, int(k)), dtype=torch.int32, device=q_offsets.device)
            score = torch.empty((nq, int(k)), dtype=torch.float64, device=q_offsets.device)
            check(lib().strsim_extract_device(self._h, measure_id(scorer), q_offsets.data_ptr(), q_values.data_ptr(), nq,
                                              c_offsets.data_ptr(), c_values.data_ptr(), nc, int(k), cut, index.data_ptr(), score.data_ptr()))
            return index, score
        qo, qv, nq = _host_column(q_offsets, q_values)
        co, cv, nc = _host_column(c_offsets, c_values)
        index = np.empty((nq, int(k)), dtype=np.uint32)
        score = np.empty((nq, int(k)), dtype=np.float64)
        check(lib().strsim_extract_host(self._h, measure_id(scorer), qo.ctypes.data, qv.ctypes.data, nq,
                                        co.ctypes.data, cv.ctypes.data, nc, int(k), cut, index.ctypes.data, score.ctypes.data))
        return index, score

    def cdist(self, measure, q_offsets, q_values, c_offsets, c_values, score_cutoff=None, out=None):
        """The full score matrix (strsim_cdist_host for numpy columns, strsim_cdist_device for torch tensors on this context's
        device): uint32 offsets + uint8 values of the queries and the candidates -> f64 [rows, candidates], element (i, j) bit for
        bit the pairwise score of (queries[i], candidates[j]) by one of the reference measures, "indel" or "token_sort_ratio"; a
        score below score_cutoff is stored as 0.0 (None: no cutoff).  `out`: a 2-D f64 array / tensor of that shape to fill, with
        unit stride along a row and any row stride >= candidates (what lies between two rows is never written).  Device inputs give
        a device output, complete in stream order."""
        cut = -np.inf if score_cutoff is None else float(score_cutoff)
        if not isinstance(q_offsets, np.ndarray) and hasattr(q_offsets, "data_ptr"):
            import torch
            nq, nc = max(q_offsets.numel() - 1, 0), max(c_offsets.numel() - 1, 0)
            if out is None:
                out = torch.empty((nq, nc), dtype=torch.float64, device=q_offsets.device)
            if out.dtype != torch.float64 or tuple(out.shape) != (nq, nc) or (nc > 1 and out.stride(1) != 1):
                raise ValueError(f"out must be a float64 tensor of shape ({nq}, {nc}) with unit stride along a row")
            ld = out.stride(0) if nq > 1 else nc
            check(lib().strsim_cdist_device(self._h, measure_id(measure), q_offsets.data_ptr(), q_values.data_ptr(), nq,
                                            c_offsets.data_ptr(), c_values.data_ptr(), nc, cut, out.data_ptr(), max(ld, nc)))
            return out
        qo, qv, nq = _host_column(q_offsets, q_values)
        co, cv, nc = _host_column(c_offsets, c_values)
        if out is None:
            out = np.empty((nq, nc), dtype=np.float64)
        if out.dtype != np.float64 or out.shape != (nq, nc) or (nc > 1 and out.strides[1] != 8) or (nq > 1 and out.strides[0] % 8):
            raise ValueError(f"out must be a float64 array of shape ({nq}, {nc}) with unit stride along a row")
        ld = out.strides[0] // 8 if nq > 1 else nc
        check(lib().strsim_cdist_host(self._h, measure_id(measure), qo.ctypes.data, qv.ctypes.data, nq,
                                      co.ctypes.data, cv.ctypes.data, nc, cut, out.ctypes.data, max(ld, nc)))
        return out

    def join(self, scorer, q_offsets, q_values, c_offsets, c_values, score_cutoff=None, upper=False, capacity=None, count_only=False):
        """Threshold join (strsim_join_host for numpy columns, strsim_join_device for torch tensors on this context's device): every
        pair (i, j) with score >= score_cutoff by "indel" or "token_sort_ratio" (None: every pair), as CSR -> (indptr [rows + 1],
        index [nnz], score f64 [nnz]); the hits of query i are index / score[indptr[i]:indptr[i + 1]], in ascending candidate index,
        the score bit for bit the pairwise call's.  upper=True reports only j > i (pass one column twice: a self-join).  The call is
        made with `capacity` slots (None: a guess from the rows) and, when the hits do not fit, once more with exactly nnz.
        count_only=True makes the count-only call and returns indptr alone.  numpy in: uint64 / uint32 / f64 arrays out; device
        tensors in: int64 / int32 / f64 tensors out, complete in stream order."""
        return self._join("strsim_join", scorer, q_offsets, q_values, c_offsets, c_values, score_cutoff, upper, capacity, count_only)

    def match_join(self, measure, q_offsets, q_values, c_offsets, c_values, min_score=None, upper=False, capacity=None, count_only=False):
        """Threshold join by one of the five reference measures (strsim_match_join_host for numpy columns, strsim_match_join_device
        for torch tensors on this context's device): every pair (i, j) with score >= min_score (None: every pair), as CSR.  The
        result, `upper`, the capacity protocol and count_only are join()'s."""
        return self._join("strsim_match_join", measure, q_offsets, q_values, c_offsets, c_values, min_score, upper, capacity, count_only)

    def qgram_join(self, kind, q_offsets, q_values, c_offsets, c_values, min_score=None, upper=False, q=2, multiset=True, capacity=None,
                   count_only=False):
        """Threshold join by q-gram similarity (strsim_qgram_join_host for numpy columns, strsim_qgram_join_device for torch tensors
        on this context's device): every pair (i, j) whose score by `kind` (one of QGRAM_KINDS) over q-grams (q: 1, 2 or 3;
        multiset=False compares the sets of grams) is >= min_score (None: every pair), as CSR; the score is bit for bit
        qgram_device's.  The result, `upper`, the capacity protocol and count_only are join()'s."""
        return self._join("strsim_qgram_join", qgram_args(kind, q, multiset), q_offsets, q_values, c_offsets, c_values, min_score, upper, capacity,
                          count_only)

    def distance_join(self, kind, q_offsets, q_values, c_offsets, c_values, max_distance=None, upper=False, capacity=None, count_only=False):
        """Join by integer edit distance (strsim_distance_join_host for numpy columns, strsim_distance_join_device for torch tensors
        on this context's device): every pair (i, j) with d(i, j) <= max_distance (None: every pair) by `kind` (one of EDIT_KINDS),
        as CSR -> (indptr [rows + 1], index [nnz], distance uint32 [nnz]; device tensors: int32); d is exactly the pairwise
        distance call's.  `upper`, the capacity protocol and count_only are join()'s."""
        return self._join("strsim_distance_join", (edit_kind_id(kind),), q_offsets, q_values, c_offsets, c_values, _max_distance(max_distance), upper,
                          capacity, count_only, values="u")

    def _join(self, entry, scorer, q_offsets, q_values, c_offsets, c_values, score_cutoff, upper, capacity, count_only, values="f"):
        """join(), match_join(), qgram_join() and distance_join(): the entry points `entry`_device / `entry`_host under the capacity
        protocol.  scorer: a measure, or the (kind id, q, flags) of a q-gram call, or the (kind id,) of a distance join, whose cutoff
        is the integer itself and whose values are uint32 (values="u")"""
        what = scorer if isinstance(scorer, tuple) else (measure_id(scorer),)
        cut = score_cutoff if values == "u" else -np.inf if score_cutoff is None else float(score_cutoff)
        flags = JOIN_UPPER if upper else 0
        nnz = C.c_uint64(0)
        device = not isinstance(q_offsets, np.ndarray) and hasattr(q_offsets, "data_ptr")
        if device:
            import torch
            nq, nc = max(q_offsets.numel() - 1, 0), max(c_offsets.numel() - 1, 0)
            cols = (q_offsets.data_ptr(), q_values.data_ptr(), nq, c_offsets.data_ptr(), c_values.data_ptr(), nc)
            fn = getattr(lib(), entry + "_device")
            indptr = torch.empty(nq + 1, dtype=torch.int64, device=q_offsets.device)
            new = lambda n, dt: torch.empty(n, dtype={"i": torch.int32, "u": torch.int32, "f": torch.float64}[dt], device=q_offsets.device)
            ptr = lambda t: t.data_ptr()
        else:
            qo, qv, nq = _host_column(q_offsets, q_values)
            co, cv, nc = _host_column(c_offsets, c_values)
            nq, nc = max(nq, 0), max(nc, 0)
            cols = (qo.ctypes.data, qv.ctypes.data, nq, co.ctypes.data, cv.ctypes.data, nc)
            fn = getattr(lib(), entry + "_host")
            indptr = np.empty(nq + 1, dtype=np.uint64)
            new = lambda n, dt: np.empty(n, dtype={"i": np.uint32, "u": np.uint32, "f": np.float64}[dt])
            ptr = lambda a: a.ctypes.data
        if count_only:
            check(fn(self._h, *what, *cols, cut, flags, 0, ptr(indptr), None, None, C.byref(nnz)))
            return indptr
        cap = 4 * nq + 1024 if capacity is None else int(capacity)
        for _ in range(2):
            index, score = new(cap, "i"), new(cap, values)
            check(fn(self._h, *what, *cols, cut, flags, cap, ptr(indptr), ptr(index) if cap else None,
                     ptr(score) if cap else None, C.byref(nnz)))
            if nnz.value <= cap:
                return indptr, index[:nnz.value], score[:nnz.value]
            cap = nnz.value  # the hits did not fit: nothing was written; once more with the exact size
        raise StrsimError(7, f"{entry}: nnz changed between two calls on the same columns ({nnz.value} > {cap})")

    def components(self, indptr, index, rows=None):
        """Connected components of a CSR graph (strsim_components_host for numpy arrays, strsim_components_device for torch tensors
        on this context's device): the edges (i, index[e]), e in [indptr[i], indptr[i + 1]), read as undirected -> (root [rows],
        cluster [rows], count).  root[v] is the smallest row of v's component, cluster[v] the number of roots below it (clusters are
        numbered in order of their first member), count the number of components.  rows=None: len(indptr) - 1.  indptr is uint64 /
        int64, index uint32 / int32.  numpy in: uint32 arrays out; device tensors in: int32 tensors out.  The call waits once."""
        count = C.c_uint64(0)
        if not isinstance(indptr, np.ndarray) and hasattr(indptr, "data_ptr"):
            import torch
            n = max(indptr.numel() - 1, 0) if rows is None else int(rows)
            nnz = index.numel()
            if indptr.numel() != n + 1 or indptr.dtype != torch.int64 or index.dtype != torch.int32:
                raise ValueError(f"components: indptr must be an int64 tensor of {n + 1} words and index an int32 tensor")
            root = torch.empty(n, dtype=torch.int32, device=indptr.device)
            cluster = torch.empty(n, dtype=torch.int32, device=indptr.device)
            check(lib().strsim_components_device(self._h, n, indptr.data_ptr(), index.data_ptr() if nnz else None, nnz,
                                                 root.data_ptr() if n else None, cluster.data_ptr() if n else None, C.byref(count)))
            return root, cluster, int(count.value)
        ip = np.ascontiguousarray(indptr).astype(np.uint64, copy=False)
        ix = np.ascontiguousarray(index).astype(np.uint32, copy=False)
        n = max(ip.size - 1, 0) if rows is None else int(rows)
        if ip.size != n + 1:
            raise ValueError(f"components: indptr must hold rows + 1 = {n + 1} words, got {ip.size}")
        root, cluster = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        check(lib().strsim_components_host(self._h, n, ip.ctypes.data, ix.ctypes.data if ix.size else None, ix.size,
                                           root.ctypes.data if n else None, cluster.ctypes.data if n else None, C.byref(count)))
        return root, cluster, int(count.value)

    def cluster(self, measure, offsets, values, min_score, with_nnz=False):
        """The duplicate groups of one column (strsim_cluster_host for numpy columns, strsim_cluster_device for torch tensors on this
        context's device): the upper self-join of the column at min_score by `measure` (one of the five reference measures, "indel"
        or "token_sort_ratio"), then the components of its hits -> (root, cluster, count) as components() returns them; the pairs
        never reach the host.  with_nnz=True appends the number of pairs."""
        count, nnz = C.c_uint64(0), C.c_uint64(0)
        if not isinstance(offsets, np.ndarray) and hasattr(offsets, "data_ptr"):
            import torch
            n = max(offsets.numel() - 1, 0)
            root = torch.empty(n, dtype=torch.int32, device=offsets.device)
            cluster = torch.empty(n, dtype=torch.int32, device=offsets.device)
            check(lib().strsim_cluster_device(self._h, measure_id(measure), offsets.data_ptr(), values.data_ptr(), n, float(min_score),
                                              root.data_ptr() if n else None, cluster.data_ptr() if n else None, C.byref(count), C.byref(nnz)))
        else:
            o, v, n = _host_column(offsets, values)
            n = max(n, 0)
            root, cluster = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
            check(lib().strsim_cluster_host(self._h, measure_id(measure), o.ctypes.data, v.ctypes.data, n, float(min_score),
                                            root.ctypes.data if n else None, cluster.ctypes.data if n else None, C.byref(count), C.byref(nnz)))
        out = (root, cluster, int(count.value))
        return out + (int(nnz.value),) if with_nnz else out

    def qgram_cluster(self, kind, offsets, values, min_score, q=2, multiset=True, with_nnz=False):
        """The duplicate groups of one column by q-gram similarity (strsim_qgram_cluster_host for numpy columns,
        strsim_qgram_cluster_device for torch tensors on this context's device): cluster() with the self-join of qgram_join(kind, q,
        multiset)."""
        kid, q, flags = qgram_args(kind, q, multiset)
        count, nnz = C.c_uint64(0), C.c_uint64(0)
        if not isinstance(offsets, np.ndarray) and hasattr(offsets, "data_ptr"):
            import torch
            n = max(offsets.numel() - 1, 0)
            root = torch.empty(n, dtype=torch.int32, device=offsets.device)
            cluster = torch.empty(n, dtype=torch.int32, device=offsets.device)
            check(lib().strsim_qgram_cluster_device(self._h, kid, q, flags, offsets.data_ptr(), values.data_ptr(), n, float(min_score),
                                                    root.data_ptr() if n else None, cluster.data_ptr() if n else None, C.byref(count),
                                                    C.byref(nnz)))
        else:
            o, v, n = _host_column(offsets, values)
            n = max(n, 0)
            root, cluster = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
            check(lib().strsim_qgram_cluster_host(self._h, kid, q, flags, o.ctypes.data, v.ctypes.data, n, float(min_score),
                                                  root.ctypes.data if n else None, cluster.ctypes.data if n else None, C.byref(count),
                                                  C.byref(nnz)))
        out = (root, cluster, int(count.value))
        return out + (int(nnz.value),) if with_nnz else out

    def distance_cluster(self, kind, offsets, values, max_distance, with_nnz=False):
        """The duplicate groups of one column by edit distance (strsim_distance_cluster_host for numpy columns,
        strsim_distance_cluster_device for torch tensors on this context's device): cluster() with the self-join of
        distance_join(kind, max_distance); None is no cutoff (one cluster)."""
        kid, k = edit_kind_id(kind), _max_distance(max_distance)
        count, nnz = C.c_uint64(0), C.c_uint64(0)
        if not isinstance(offsets, np.ndarray) and hasattr(offsets, "data_ptr"):
            import torch
            n = max(offsets.numel() - 1, 0)
            root = torch.empty(n, dtype=torch.int32, device=offsets.device)
            cluster = torch.empty(n, dtype=torch.int32, device=offsets.device)
            check(lib().strsim_distance_cluster_device(self._h, kid, offsets.data_ptr(), values.data_ptr(), n, k, root.data_ptr() if n else None,
                                                       cluster.data_ptr() if n else None, C.byref(count), C.byref(nnz)))
        else:
            o, v, n = _host_column(offsets, values)
            n = max(n, 0)
            root, cluster = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
            check(lib().strsim_distance_cluster_host(self._h, kid, o.ctypes.data, v.ctypes.data, n, k, root.ctypes.data if n else None,
                                                     cluster.ctypes.data if n else None, C.byref(count), C.byref(nnz)))
        out = (root, cluster, int(count.value))
        return out + (int(nnz.value),) if with_nnz else out

class Codec:
    """Lossless 16-bit transport codec for one measure's result column (include/strsim_amd.h: strsim_codec_*)."""
    EXC_CAP = 1 << 20

    def __init__(self, ctx, measure, max_chars=32):
        import torch
        self.ctx = ctx
        self._h = C.c_void_p()
        check(lib().strsim_codec_create(ctx._h, measure_id(measure), int(max_chars), C.byref(self._h)))
        dev = torch.device("cuda", ctx.device)
        self.exc_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.exc_rows = torch.empty(self.EXC_CAP, dtype=torch.int32, device=dev)
        self.exc_vals = torch.empty(self.EXC_CAP, dtype=torch.float64, device=dev)

    @property
    def entries(self):
        return int(lib().strsim_codec_entries(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().strsim_codec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _exc(self, exc):
        """(count ptr, rows ptr, vals ptr, cap) of an exception block: this codec's own, or `exc` = (count, rows, vals)
        tensors of the caller (e.g. views into a buffer that is shipped together with the codes)."""
        if exc is None:
            return self.exc_count.data_ptr(), self.exc_rows.data_ptr(), self.exc_vals.data_ptr(), self.EXC_CAP
        cnt, rows, vals = exc
        return cnt.data_ptr(), rows.data_ptr(), vals.data_ptr(), min(rows.numel(), vals.numel())

    def encode(self, vals, codes=None, ctx=None, exc=None):
        """f64 tensor -> int16 tensor of codes (0xFFFF = exception, see exc_*); asynchronous on ctx's stream."""
        import torch
        ctx = ctx or self.ctx
        if codes is None:
            codes = torch.empty(vals.numel(), dtype=torch.int16, device=vals.device)
        pc, pr, pv, cap = self._exc(exc)
        check(lib().strsim_codec_encode(ctx._h, self._h, vals.data_ptr(), vals.numel(), codes.data_ptr(), pc, pr, pv, cap))
        return codes

    def decode(self, codes, out=None, ctx=None):
        import torch
        ctx = ctx or self.ctx
        if out is None:
            out = torch.empty(codes.numel(), dtype=torch.float64, device=codes.device)
        check(lib().strsim_codec_decode(ctx._h, self._h, codes.data_ptr(), codes.numel(), out.data_ptr()))
        return out

    @property
    def bits(self):
        """Bits per row of the packed transport (2^bits > entries; the all-ones code is the escape)."""
        return int(lib().strsim_codec_bits(self._h))

    def packed_words(self, n):
        return int(lib().strsim_codec_packed_words(self._h, int(n)))

    def encode_packed(self, vals, words=None, ctx=None, exc=None):
        """f64 tensor -> int64 tensor of packed_words(n) words, 64 // bits codes each; asynchronous on ctx's stream."""
        import torch
        ctx = ctx or self.ctx
        if words is None:
            words = torch.empty(self.packed_words(vals.numel()), dtype=torch.int64, device=vals.device)
        pc, pr, pv, cap = self._exc(exc)
        check(lib().strsim_codec_encode_packed(ctx._h, self._h, vals.data_ptr(), vals.numel(), words.data_ptr(), pc, pr, pv, cap))
        return words

    def decode_packed(self, words, n, out=None, ctx=None):
        import torch
        ctx = ctx or self.ctx
        if out is None:
            out = torch.empty(int(n), dtype=torch.float64, device=words.device)
        check(lib().strsim_codec_decode_packed(ctx._h, self._h, words.data_ptr(), int(n), out.data_ptr()))
        return out

    def patch_indirect(self, out, row_base, exc, overflow, ctx=None):
        """out[row_base + rows[i]] = vals[i] for i < min(count, cap), the count read on the device; `exc` = (count, rows, vals)
        tensors (an exception block as it arrived from another rank), `overflow`: int32 device tensor, incremented when
        count > cap."""
        ctx = ctx or self.ctx
        cnt, rows, vals = exc
        check(lib().strsim_codec_patch_indirect(ctx._h, out.data_ptr(), int(row_base), cnt.data_ptr(), rows.data_ptr(),
                                                vals.data_ptr(), min(rows.numel(), vals.numel()), overflow.data_ptr()))

    def decode_gathered(self, buf, seg_stride_bytes, nseg, chunk_rows, last_rows, packed, code_bytes, exc_cap, out, overflow, ctx=None,
                        first_seg=0):
        """The root's decode of every rank's segment of a gathered buffer (codes + exception block each) in ONE launch:
        strsim_codec_decode_gathered; `first_seg` = 1 leaves the root's own segment alone (strsim_codec_decode_gathered_from: the
        root copies its f64 shard in instead of coding and decoding it)."""
        ctx = ctx or self.ctx
        check(lib().strsim_codec_decode_gathered_from(ctx._h, self._h, buf.data_ptr(), int(seg_stride_bytes), int(first_seg), int(nseg),
                                                      int(chunk_rows), int(last_rows), 1 if packed else 0, int(code_bytes), int(exc_cap),
                                                      out.data_ptr(), overflow.data_ptr()))

    def patch(self, out, row_base, exc_rows, exc_vals, count, ctx=None):
        ctx = ctx or self.ctx
        check(lib().strsim_codec_patch(ctx._h, out.data_ptr(), int(row_base), exc_rows.data_ptr(), exc_vals.data_ptr(),
                                       int(count)))


def _host_column(offsets, values):
    """-> (contiguous uint32 offsets, contiguous uint8 values with one padding byte when empty, rows)"""
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    val = np.ascontiguousarray(values, dtype=np.uint8)
    if val.size == 0:
        val = np.zeros(1, dtype=np.uint8)
    return off, val, off.size - 1


def _rows_out(ra, rb):
    """Rows an elementwise call produces; 0 for a shape the library is going to refuse (it reports the error)."""
    if ra != rb and ra != 1 and rb != 1:
        return 0
    return rb if ra == 1 else ra


def _check_device_column(offsets, values):
    assert offsets.is_cuda and offsets.element_size() == 4 and offsets.is_contiguous()
    assert values.is_cuda and values.element_size() == 1 and values.is_contiguous()


def _max_distance(k):
    """None -> STRSIM_DISTANCE_UNBOUNDED; else an int in 0 .. 2^32 - 1."""
    if k is None:
        return DISTANCE_UNBOUNDED
    k = int(k)
    if not 0 <= k <= DISTANCE_UNBOUNDED:
        raise ValueError(f"max_distance={k} is outside 0 .. {DISTANCE_UNBOUNDED}")
    return k


def pack_strings(strings):
    """list[str|bytes] -> (uint32 offsets[n+1], uint8 values): the device column layout."""
    bs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]
    offs = np.zeros(len(bs) + 1, dtype=np.uint32)
    if bs:
        offs[1:] = np.cumsum([len(x) for x in bs], dtype=np.uint64).astype(np.uint32)
    vals = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, dtype=np.uint8)
    return offs, vals
