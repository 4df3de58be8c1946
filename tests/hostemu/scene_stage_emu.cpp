// Host build of csrc/scene_stage.h for tests/test_scene_stage.py: the rule the entry points of csrc/polytope_lp.hip call, by call number.
// Test infrastructure: never shipped, never timed.
#include "scene_stage.h"
using namespace gcsadmm_stage;

extern "C" {

int stage_emu_calls(void) { return CALL_COUNT; }
// the refusal of `call` on a scene with the results `have`, or a null pointer
const char *stage_emu_need(unsigned have, int call) { return need(have, (Call)call); }
unsigned stage_emu_after(unsigned have, int call, int finished) { return stage_after(have, (Call)call, finished != 0); }
// ... as the entry points apply it
unsigned stage_emu_start(unsigned have, int call) { stage_start(have, (Call)call); return have; }
unsigned stage_emu_finish(unsigned have, int call) { stage_finish(have, (Call)call); return have; }

} // extern "C"
