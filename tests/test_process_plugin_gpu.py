"""The default_process plugin function end to end on the GPU, with pyarrow standing in for the Polars engine
(strsim_amd.arrow_host): the result type and field, values against tests/process_ref.py, nulls, a sliced input, chunks, the three
input layouts, zero rows, and who releases what."""
import gc

import pyarrow as pa
import pytest

import process_frames as F
import process_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from strsim_amd import arrow_host
    return arrow_host


def column():
    rows = list(F.frame()[:1500]) + ["Apple, Inc.", "!!!", "", "ȺȾ" * 50]
    for i in range(0, len(rows), 29):
        rows[i] = None
    return rows


def test_type_field_and_name(H):
    probe = {}
    got = H.call_plugin_unary("default_process", ["Apple, Inc.", None, "ÀÉ　x"], input_name="company", _probe=probe)
    assert got.type == pa.string() and got.to_pylist() == ["apple  inc", None, "àé x"]
    assert probe["name"] == "company" and probe["format"] == "u"
    assert H.field_plugin("default_process", ("company",)) == ("company", pa.string())


@pytest.mark.parametrize("layout", ["vu", "u", "U"])
def test_values_nulls_chunks_and_slices(H, layout):
    rows = column()
    want = [R.default_process(s) for s in rows]
    arr = pa.array(rows, pa.string())
    got = H.call_plugin_unary("default_process", arr, layout=layout)
    assert got.num_chunks == 1 and got.null_count == sum(s is None for s in rows)
    assert got.to_pylist() == want
    chunked = pa.chunked_array([arr[:7], arr[7:700], arr[700:700], arr[700:]])
    assert H.call_plugin_unary("default_process", chunked, layout=layout).to_pylist() == want
    padded = pa.array(["Pad, "] * 3 + rows + [None] * 5, pa.string())[3:3 + len(rows)]   # a sliced input: offset 3
    assert H.call_plugin_unary("default_process", padded, layout=layout).to_pylist() == want
    assert H.call_plugin_unary("default_process", arr[1:2], layout=layout).to_pylist() == want[1:2]


@pytest.mark.parametrize("layout", ["vu", "u", "U"])
def test_zero_rows_and_all_null(H, layout):
    got = H.call_plugin_unary("default_process", pa.array([], pa.string()), layout=layout)
    assert got.type == pa.string() and got.to_pylist() == []
    assert H.call_plugin_unary("default_process", [None, None, None], layout=layout).to_pylist() == [None] * 3


def test_released_exactly_once(H):
    probe = {}
    got = H.call_plugin_unary("default_process", column(), _probe=probe)
    assert probe["series_released"] == [1] and probe["arrays_released"] == [True]      # the callee released its input, once
    assert probe["arrays_moved"] and probe["series_released_after"]                   # the importer took the result's array
    assert len(got.to_pylist()) == len(column())
    del got
    gc.collect()  # the array's release callback frees the three buffers here; a second release would be a double free
    again = H.call_plugin_unary("default_process", ["B, a"])
    assert again.to_pylist() == ["b  a"]


def test_wrong_inputs(H):
    with pytest.raises(H.PluginError, match="expected `String`"):
        H.call_plugin_unary("default_process", pa.array([1, 2, 3], pa.int64()))
    with pytest.raises(H.PluginError, match="default_process: expected 1 input series, got 2"):
        H.call_plugin("default_process", ["a"], ["b"])
