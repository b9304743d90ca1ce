"""The results the plugin functions hand back, without a GPU: every exported family's Arrow type, length, nulls and ownership.

A call whose every row is null (a null literal) or that has no rows never opens a context, so it runs on a machine without a
device and still goes through the whole result export: the struct of best match, nearest match and partial_ratio_alignment (what
a consumer may move out, what is freed when) and the one-chunk primitive result of the similarity and distance functions.

The result is imported with the type the plugin itself reports in the returned field, not with one the test supplies.  The
expectations were checked against the library of the commit before the plugin's result export was folded into one place
(a8969f6); the test passes unchanged on both sides of that change.
"""
import ctypes as C

import pyarrow as pa
import pytest

U32, F64 = pa.uint32(), pa.float64()
MATCH = pa.struct([pa.field("index", U32), pa.field("score", F64)])
NEAREST = pa.struct([pa.field("index", U32), pa.field("distance", U32)])
ALIGNMENT = pa.struct([pa.field("score", F64), pa.field("src_start", U32), pa.field("src_end", U32), pa.field("dest_start", U32),
                       pa.field("dest_end", U32)])

ELEMENTWISE = [("levenshtein", F64), ("jaro", F64), ("osa", F64), ("indel", F64), ("partial_ratio", F64),
               ("levenshtein_distance", U32), ("osa_distance", U32), ("indel_distance", U32), ("partial_ratio_alignment", ALIGNMENT)]
SEARCH = [("best_match_" + m, MATCH) for m in ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")] + \
         [("nearest_" + m, NEAREST) for m in ("levenshtein", "osa")]


def call(name, a, b, layout="vu", names=("left", "right")):
    """One plugin call the way the engine makes it -> (field name, pyarrow array of the type the plugin reports, probe)."""
    from strsim_amd import arrow_host as H
    from strsim_amd import lib
    L = lib()
    fn = getattr(L, "_polars_plugin_" + name)
    fn.restype = None
    fn.argtypes = [C.POINTER(H.SeriesExport), C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(H.SeriesExport), C.POINTER(H.CallerContext)]
    L._polars_plugin_get_last_error_message.restype = C.c_char_p
    inputs = (H.SeriesExport * 2)()
    exported = []
    for i, x in enumerate((a, b)):
        chunks, dtype = H._chunks(x, layout)
        ex = H._Exported(names[i], chunks, dtype)
        ex.fill(inputs[i])
        exported.append(ex)
    ret = H.SeriesExport()
    fn(inputs, 2, None, 0, C.byref(ret), C.byref(H.CallerContext(0)))
    probe = {"series_released": [e.released for e in exported], "arrays_released": [e.arrays_released() for e in exported]}
    assert ret.private_data, L._polars_plugin_get_last_error_message().decode()
    try:
        assert ret.len == 1
        field = pa.Field._import_from_c(C.addressof(ret.field.contents))  # (moved out: the series releases what is left)
        arr = pa.Array._import_from_c(C.addressof(ret.arrays[0].contents), field.type)
    finally:
        ret.release(C.byref(ret))
    arr.validate(full=True)
    return field, arr, probe


def check(name, typ, field, arr, probe, rows):
    """`rows` rows, every one null, of the family's type named after input 0; both inputs released exactly once."""
    from strsim_amd import arrow_host as H
    assert field.name == "left" and field.type == typ and field.nullable
    assert arr.type == typ
    if pa.types.is_struct(typ):
        assert [arr.type.field(i).name for i in range(arr.type.num_fields)] == [f.name for f in typ]
    assert len(arr) == rows and arr.null_count == rows
    assert arr.to_pylist() == [None] * rows
    if pa.types.is_struct(typ):
        for i in range(typ.num_fields):  # every child carries its own copy of the validity
            child = arr.field(i)
            assert child.type == typ.field(i).type and len(child) == rows and child.null_count == rows
            assert child.to_pylist() == [None] * rows
    assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    assert H.field_plugin(name, ("left", "right")) == ("left", typ)


@pytest.mark.parametrize("layout", ["vu", "u", "U"])
@pytest.mark.parametrize("name,typ", ELEMENTWISE)
def test_null_literal_gives_an_all_null_column(name, typ, layout):
    one_null = pa.array([None], type=pa.string())
    check(name, typ, *call(name, ["ab", "cd", None], one_null, layout), rows=3)
    check(name, typ, *call(name, one_null, ["ab", "cd"], layout), rows=2)
    check(name, typ, *call(name, one_null, one_null, layout), rows=1)


@pytest.mark.parametrize("name,typ", ELEMENTWISE)
def test_elementwise_call_without_rows(name, typ):
    check(name, typ, *call(name, [], []), rows=0)
    check(name, typ, *call(name, [], ["literal"]), rows=0)


@pytest.mark.parametrize("name,typ", SEARCH)
def test_search_without_queries_gives_an_empty_struct(name, typ):
    check(name, typ, *call(name, [], ["ab", None, "cd"]), rows=0)
    check(name, typ, *call(name, [], []), rows=0)


@pytest.mark.parametrize("name,typ", [("partial_ratio_alignment", ALIGNMENT), ("levenshtein_distance", U32), ("indel", F64)])
def test_wider_than_one_validity_word(name, typ):
    # 200 rows: four validity words, the last one partly used
    check(name, typ, *call(name, ["row %d" % i for i in range(200)], pa.array([None], type=pa.string())), rows=200)


def test_children_read_through_views_after_the_struct_is_dropped():
    # (pyarrow imports the struct whole and a child is a view that keeps it alive: this does not move a child out of the struct)
    field, arr, probe = call("partial_ratio_alignment", ["ab", "cd", None], pa.array([None], type=pa.string()))
    children = [arr.field(i) for i in range(5)]
    del arr
    for child in children:
        assert child.null_count == 3 and child.to_pylist() == [None] * 3


def test_failures_leave_no_result_and_release_the_inputs():
    from strsim_amd import arrow_host as H
    for name, typ in ELEMENTWISE:
        probe = {}
        with pytest.raises(H.PluginError, match="Inputs must have the same length, or one of them must be a Utf8 literal."):
            H.call_plugin(name, ["a", "b"], ["a", "b", "c"], _probe=probe, out_type=typ)
        assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
    for name, typ in ELEMENTWISE + SEARCH:
        probe = {}
        with pytest.raises(H.PluginError, match="invalid series dtype: expected `String`"):
            H.call_plugin(name, pa.array([1, 2]), pa.array(["a", "b"]), _probe=probe, out_type=typ)
        assert probe["series_released"] == [1, 1] and probe["arrays_released"] == [True, True]
