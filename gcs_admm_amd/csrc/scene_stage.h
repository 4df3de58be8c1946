// scene_stage.h -- which results a resident scene holds, which of them each call needs, and which it ends: the one place that says so
// (plain C++: polytope_lp.hip calls it, tests/hostemu/scene_stage_emu.cpp compiles it for tests/test_scene_stage.py).  The results
// are six flags in one word.  A call asks need() first (the first missing result of its row refuses it, nothing changed), clears
// its "start" set once its arguments are accepted, and clears its "finish" set and sets its "sets" set when its last step has
// succeeded -- so a call that fails half way leaves its "start" set cleared.
//
//   call              needs (in this order)             start clears             finish clears   sets
//   centers           -                                 centers                  -               centers
//   bounds            centers                           boxes, pairs, overlaps   -               boxes
//   set_boxes         -                                 boxes, pairs, overlaps   -               boxes
//   candidate_pairs   boxes                             pairs, overlaps, graph   -               pairs
//   overlaps          pairs, centers                    overlaps, graph          -               overlaps
//   locate_points     -                                 hits                     -               hits          (and locate_boxes: the same list)
//   add_regions       centers, boxes, pairs, decided    -                        hits, graph     -
//   remove_regions    -                                 -                        hits, graph     -
//   build_graph       decided                           -                        -               graph
//   read_centers      centers        read_boxes   boxes        read_pairs   pairs        read_decisions   pairs, decided
//   read_hits         hits           read_graph   graph        query_graphs graph (its own text)            (reads change nothing)
//
// "decided" is pairs and overlaps together.  gcsadmm_scene_restrict_paths needs the regions alone and is not in the table; nor are
// gcsadmm_scene_region_paths (NEED_FRESH_GRAPH, NEED_CENTERS), gcsadmm_scene_informed_regions (NEED_BOXES) and
// gcsadmm_scene_induced_sizes / _induced_query_graphs (NEED_FRESH_GRAPH), which read and change nothing.  An edit of no regions returns before its finish.
#pragma once

namespace gcsadmm_stage {

enum : unsigned { HAVE_CENTERS = 1, HAVE_BOXES = 2, HAVE_PAIRS = 4, HAVE_OVERLAPS = 8, HAVE_HITS = 16, HAVE_GRAPH = 32 };

enum Call {
    CALL_CENTERS, CALL_BOUNDS, CALL_SET_BOXES, CALL_CANDIDATE_PAIRS, CALL_OVERLAPS, CALL_LOCATE_POINTS, CALL_ADD_REGIONS, CALL_REMOVE_REGIONS,
    CALL_BUILD_GRAPH, CALL_READ_CENTERS, CALL_READ_BOXES, CALL_READ_PAIRS, CALL_READ_DECISIONS, CALL_READ_HITS, CALL_READ_GRAPH,
    CALL_QUERY_GRAPHS, CALL_COUNT
};

// what a call can need: the flags that must all be set, and the refusal when one is not
struct NeedRule { unsigned flags; const char *refusal; };
constexpr NeedRule NEED_CENTERS{HAVE_CENTERS, "no resident centres: call gcsadmm_scene_centers first"},
    NEED_BOXES{HAVE_BOXES, "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first"},
    NEED_PAIRS{HAVE_PAIRS, "no resident pairs: call gcsadmm_scene_candidate_pairs first"},
    NEED_DECIDED{HAVE_PAIRS | HAVE_OVERLAPS, "the resident pairs are not decided: call gcsadmm_scene_overlaps first"},
    NEED_HITS{HAVE_HITS, "no resident hit list: call gcsadmm_scene_locate_points first"},
    NEED_GRAPH{HAVE_GRAPH, "no resident region graph: call gcsadmm_scene_build_region_graph first"},
    NEED_FRESH_GRAPH{HAVE_GRAPH, "no resident region graph, or one from before an edit: call gcsadmm_scene_build_region_graph first"};

struct StageRule { NeedRule needs[4]; unsigned start_clears, finish_clears, sets; };
inline StageRule stage_rule(Call call)
{
    switch (call) {
    case CALL_CENTERS: return {{}, HAVE_CENTERS, 0, HAVE_CENTERS};
    case CALL_BOUNDS: return {{NEED_CENTERS}, HAVE_BOXES | HAVE_PAIRS | HAVE_OVERLAPS, 0, HAVE_BOXES};
    case CALL_SET_BOXES: return {{}, HAVE_BOXES | HAVE_PAIRS | HAVE_OVERLAPS, 0, HAVE_BOXES};
    case CALL_CANDIDATE_PAIRS: return {{NEED_BOXES}, HAVE_PAIRS | HAVE_OVERLAPS | HAVE_GRAPH, 0, HAVE_PAIRS};
    case CALL_OVERLAPS: return {{NEED_PAIRS, NEED_CENTERS}, HAVE_OVERLAPS | HAVE_GRAPH, 0, HAVE_OVERLAPS};
    case CALL_LOCATE_POINTS: return {{}, HAVE_HITS, 0, HAVE_HITS};
    case CALL_ADD_REGIONS: return {{NEED_CENTERS, NEED_BOXES, NEED_PAIRS, NEED_DECIDED}, 0, HAVE_HITS | HAVE_GRAPH, 0};
    case CALL_REMOVE_REGIONS: return {{}, 0, HAVE_HITS | HAVE_GRAPH, 0};
    case CALL_BUILD_GRAPH: return {{NEED_DECIDED}, 0, 0, HAVE_GRAPH};
    case CALL_READ_CENTERS: return {{NEED_CENTERS}, 0, 0, 0};
    case CALL_READ_BOXES: return {{NEED_BOXES}, 0, 0, 0};
    case CALL_READ_PAIRS: return {{NEED_PAIRS}, 0, 0, 0};
    case CALL_READ_DECISIONS: return {{NEED_PAIRS, NEED_DECIDED}, 0, 0, 0};
    case CALL_READ_HITS: return {{NEED_HITS}, 0, 0, 0};
    case CALL_READ_GRAPH: return {{NEED_GRAPH}, 0, 0, 0};
    case CALL_QUERY_GRAPHS: return {{NEED_FRESH_GRAPH}, 0, 0, 0};
    default: return {{}, 0, 0, 0};
    }
}

inline bool has(unsigned have, unsigned flags) { return (have & flags) == flags; }

// nullptr: the call may run; otherwise the text of the refusal (GCSADMM_ERR_BAD_ARG), the first of the row that applies
inline const char *need(unsigned have, Call call)
{
    const StageRule rule = stage_rule(call);
    for (const NeedRule &r : rule.needs)      // (an empty place of the row needs nothing)
        if (!has(have, r.flags)) return r.refusal;
    return nullptr;
}

// the flags after `call` has started (finished == false) or has finished, from the flags before
inline unsigned stage_after(unsigned have, Call call, bool finished)
{
    const StageRule rule = stage_rule(call);
    return finished ? ((have & ~rule.finish_clears) | rule.sets) : (have & ~rule.start_clears);
}
inline void stage_start(unsigned &have, Call call) { have = stage_after(have, call, false); }
inline void stage_finish(unsigned &have, Call call) { have = stage_after(have, call, true); }

} // namespace gcsadmm_stage
