"""One name per first kernel of a pairwise call, and how a test reaches it through the public Python surface.

The launcher's rule is launch_lane_t and launch_lane_all_only in polars-strsim_amd/csrc/strsim_kernels.hip; the state it reads is
set in strsim_capi.cpp (ctx_retire_slot: expect_slow, long_rows; strsim_ctx_create: STRSIM_NO_LITERAL_PATH).  No counter tells
which instantiation ran: profiles/stage_routes_kernels.txt is the kernel trace of tests/test_stage_routes_gpu.py that shows every
name below reached.

  route     kernels                                                             reached by                                  cap
  plain     k_lane_stage<levenshtein,0,0,1>, <jaccard,0,0>, <sorensen_dice,0,0>  both sides > 1 row, fresh context          10 240
  tables    k_lane_stage<jaro,1,0>, <jaro_winkler,1,0>, k_lane_stage_all        the same (ALL: pairs_device_all)            8 960
  long      k_lane_stage<M,0,1>, five measures                                  the same, on a primed context              15 104
  nolit     k_lane_stage<M,T,0>, five measures, and k_lane_stage_all once       a one-row side, STRSIM_NO_LITERAL_PATH=1   the column side's
  lit       k_lane_lit<M>, five measures                                        a one-row side                             10 240

A fresh one-launch context enqueues the first kernel alone (1 operation; the literal kernel has k_publish_lit behind it: 2) and
reports what that kernel left to the later ones as last_late_rows.  A primed context expects slow rows: its next call enqueues all
five operations (6 on the literal route) and the rows the first kernel leaves are finished in stream order, uncounted.
"""
from collections import namedtuple

import stage_frames as F

ALL = "all"  # the five-output pass: Context.pairs_device_all

# kind: whose block cut (stage_frames.ranges); sides: the literal sides a test runs (None: two columns); env: set before the context
# is created; primed: the long-row geometry; ops: operations the call enqueues on a fresh (primed: a primed) one-launch context
Route = namedtuple("Route", "name measure cap kind sides env primed ops kernel")

TABLE_MEASURES = ("jaro", "jaro_winkler", ALL)  # STRSIM_STAGE_LUT 0x26
MEASURES = ("levenshtein", "jaro", "jaro_winkler", "jaccard", "sorensen_dice")


def _cap(measure):
    return F.CAP_TABLES if measure in TABLE_MEASURES else F.CAP_PLAIN


def _routes():
    out = []
    for m in MEASURES + (ALL,):
        name = "tables" if m in TABLE_MEASURES else "plain"
        kernel = "k_lane_stage_all" if m == ALL else "k_lane_stage<%s,%d,0%s>" % (m, m in TABLE_MEASURES, ",1" if m == "levenshtein" else "")
        out.append(Route(name, m, _cap(m), "stage", (None,), {}, False, 1, kernel))
    for m in MEASURES:
        out.append(Route("long", m, F.CAP_LONG, "stage", (None,), {}, True, 5, "k_lane_stage<%s,0,1>" % m))
    for m in MEASURES + (ALL,):
        kernel = "k_lane_stage_all" if m == ALL else "k_lane_stage<%s,%d,0>" % (m, m in TABLE_MEASURES)
        # (the five-output pass: once, the literal on side b)
        out.append(Route("nolit", m, _cap(m), "stage", ("b",) if m == ALL else ("a", "b"), {"STRSIM_NO_LITERAL_PATH": "1"}, False, 1, kernel))
    for m in MEASURES:
        out.append(Route("lit", m, F.CAP_LIT, "lit", ("a", "b"), {}, False, 2, "k_lane_lit<%s>" % m))
    return out


ROUTES = _routes()
FIRST_KERNELS = sorted({r.kernel for r in ROUTES})
assert len(FIRST_KERNELS) == 17


def route_id(r):
    return "%s-%s" % (r.name, r.measure)
