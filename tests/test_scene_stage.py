"""The stage rule of the resident scene (csrc/scene_stage.h, compiled for the host by tests/hostemu/scene_stage_emu.cpp): which
results each gcsadmm_scene_* call needs, in which order it asks for them and with which text it refuses, which it ends when it starts
and which it ends and sets when it has finished.  The table below is literal data, written down from the entry points as they stood
when every one of them kept its own ``have_*`` flags (polytope_lp.hip before scene_stage.h existed); it is not read from the header.
No GPU."""
from __future__ import annotations

import ctypes as C

import pytest

from hostemu_lib import emu_library


CENTERS, BOXES, PAIRS, OVERLAPS, HITS, GRAPH = 1, 2, 4, 8, 16, 32
ALL = 63

NO_CENTERS = (CENTERS, "no resident centres: call gcsadmm_scene_centers first")
NO_BOXES = (BOXES, "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first")
NO_PAIRS = (PAIRS, "no resident pairs: call gcsadmm_scene_candidate_pairs first")
NOT_DECIDED = (PAIRS | OVERLAPS, "the resident pairs are not decided: call gcsadmm_scene_overlaps first")
NO_HITS = (HITS, "no resident hit list: call gcsadmm_scene_locate_points first")
NO_GRAPH = (GRAPH, "no resident region graph: call gcsadmm_scene_build_region_graph first")
NO_FRESH_GRAPH = (GRAPH, "no resident region graph, or one from before an edit: call gcsadmm_scene_build_region_graph first")

# call number (the order of `enum Call`): name, the checks in the order the entry point makes them, cleared at the start, cleared
# at the finish, set at the finish
TABLE = [
    ("centers", [], CENTERS, 0, CENTERS),
    ("bounds", [NO_CENTERS], BOXES | PAIRS | OVERLAPS, 0, BOXES),
    ("set_boxes", [], BOXES | PAIRS | OVERLAPS, 0, BOXES),
    ("candidate_pairs", [NO_BOXES], PAIRS | OVERLAPS | GRAPH, 0, PAIRS),
    ("overlaps", [NO_PAIRS, NO_CENTERS], OVERLAPS | GRAPH, 0, OVERLAPS),
    ("locate_points", [], HITS, 0, HITS),
    ("add_regions", [NO_CENTERS, NO_BOXES, NO_PAIRS, NOT_DECIDED], 0, HITS | GRAPH, 0),
    ("remove_regions", [], 0, HITS | GRAPH, 0),
    ("build_region_graph", [NOT_DECIDED], 0, 0, GRAPH),
    ("read_regions: centres, radii or their statuses", [NO_CENTERS], 0, 0, 0),
    ("read_regions: lo or hi", [NO_BOXES], 0, 0, 0),
    ("read_pairs: the pairs alone", [NO_PAIRS], 0, 0, 0),
    ("read_pairs: flags or statuses", [NO_PAIRS, NOT_DECIDED], 0, 0, 0),
    ("read_hits", [NO_HITS], 0, 0, 0),
    ("read_region_graph", [NO_GRAPH], 0, 0, 0),
    ("query_graphs", [NO_FRESH_GRAPH], 0, 0, 0),
]
CALLS = [pytest.param(i, id=row[0].split(":")[0].replace(" ", "_") + f"_{i}") for i, row in enumerate(TABLE)]


@pytest.fixture(scope="module")
def emu():
    lib = emu_library("scenestageemu")
    lib.stage_emu_calls.restype = C.c_int
    lib.stage_emu_need.restype = C.c_char_p
    lib.stage_emu_need.argtypes = [C.c_uint, C.c_int]
    for f in (lib.stage_emu_after, lib.stage_emu_start, lib.stage_emu_finish):
        f.restype = C.c_uint
    lib.stage_emu_after.argtypes = [C.c_uint, C.c_int, C.c_int]
    lib.stage_emu_start.argtypes = lib.stage_emu_finish.argtypes = [C.c_uint, C.c_int]
    return lib


def test_the_table_names_every_call(emu):
    assert emu.stage_emu_calls() == len(TABLE)


def expected_refusal(checks, have):
    for flags, text in checks:
        if have & flags != flags:
            return text
    return None


@pytest.mark.parametrize("call", CALLS)
def test_flags_after_start_and_finish(emu, call):
    _, _, start_clears, finish_clears, sets = TABLE[call]
    for have in range(ALL + 1):      # the all-clear and the all-set word, and every word between them
        started = have & ~start_clears
        finished = (started & ~finish_clears) | sets
        assert emu.stage_emu_after(have, call, 0) == emu.stage_emu_start(have, call) == started, (have, started)
        assert emu.stage_emu_after(started, call, 1) == emu.stage_emu_finish(started, call) == finished, (have, finished)
    # spelled out for the two words: a call that fails half way leaves what it cleared at its start cleared, and sets nothing
    assert emu.stage_emu_start(0, call) == 0 and emu.stage_emu_finish(0, call) == sets
    assert emu.stage_emu_start(ALL, call) == ALL - start_clears
    assert emu.stage_emu_finish(ALL - start_clears, call) == ((ALL - start_clears) & ~finish_clears) | sets


@pytest.mark.parametrize("call", CALLS)
def test_need_refuses_with_the_first_missing_result(emu, call):
    checks = TABLE[call][1]
    assert emu.stage_emu_need(ALL, call) is None
    first = emu.stage_emu_need(0, call)
    assert (first.decode() if first else None) == (checks[0][1] if checks else None)
    for have in range(ALL + 1):
        got = emu.stage_emu_need(have, call)
        assert (got.decode() if got else None) == expected_refusal(checks, have), have
