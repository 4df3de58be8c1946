"""Properties of the compiled kernels that the design depends on, read from the compiler's resource remarks of the in-tree build
(no GPU needed: hipcc cross-compiles gfx950)."""


def test_no_kernel_uses_scratch():
    """Every kernel of the library fits the register file: no scratch (spills).  Beyond the cost (round 1: 760 B / lane made the
    vertex kernel HBM-bound on its own spills), this compiler places a spill next to a divergent branch under a partial EXEC mask
    (seen in the diagnostic timing build of the n = 6 workgroup program: every solve failed), so scratch is a correctness risk."""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    names = " ".join(res)
    for must in ("vertex_wg_kernelILi2E", "vertex_wg_kernelILi3E", "vertex_wg_kernelILi6E", "vertex_prox_kernelILi6E", "vertex_kernel",
                 "edge_kernel", "halo_pack_kernel", "ball_kernel"):
        assert must in names, must
    bad = {k: v for k, v in res.items() if v.get("scratch", 0) != 0}
    assert not bad, bad


def test_workgroup_program_occupancy():
    """registers of the workgroup program allow the residency DESIGN.md section 4 states (and the auto rule of gcsadmm_create
    relies on: 4 workgroups per CU at n = 2): n = 2, 3 four wavefronts per SIMD or more (<= 128 VGPRs), n = 6 two (<= 256), the BOX
    instantiation at n = 6 three (<= 168: its 47 KB of LDS fit a CU three times, BASELINE config 5 runs on it)"""
    from gcs_admm_amd import build
    res = build.kernel_resources()
    assert any("gcs_wg_t512" in k for k in res)        # the 512-thread build (one workgroup per CU: two wavefronts per SIMD, <= 256)
    for k, v in res.items():
        if "gcs_wg_t512" in k:
            assert v["vgprs"] + v["agprs"] <= 256, (k, v)
            continue
        if "vertex_wg_kernelILi2E" in k or "vertex_wg_kernelILi3E" in k:
            assert v["vgprs"] + v["agprs"] <= 128, (k, v)
        if "vertex_wg_kernelILi6E" in k:
            assert v["vgprs"] + v["agprs"] <= (168 if "Lb1E" in k else 256), (k, v)


def _device_disassembly(tmp_path, obj_name):
    """gfx950 disassembly of one object of the in-tree build (llvm-objdump extracts the offload bundle next to its input: a copy)"""
    import os
    import shutil
    import subprocess
    from gcs_admm_amd import build
    build.build()
    llvm = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(llvm):
        import pytest
        pytest.skip("llvm-objdump not found")
    obj = tmp_path / obj_name
    shutil.copy(os.path.join(build.HERE, obj_name), obj)
    subprocess.check_call([llvm, "--offloading", str(obj)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f and "gfx950" in f]
    assert len(dev) == 1, dev
    return subprocess.check_output([llvm, "-d", str(tmp_path / dev[0])], text=True)


def test_edge_kernel_hands_its_partials_over_with_sc1(tmp_path):
    """The last-workgroup hand-off of edge_kernel MODE 2 / 3 (csrc/loop_kernels.h, in gcsadmm.o) is relaxed agent-scope atomics + `s_waitcnt
    vmcnt(0)` -- it relies on the partials being WRITE-THROUGH stores (sc1) that are drained before the ticket add, and on the last
    workgroup reading them with sc1 loads (visible across the XCDs' L2s).  That is a property of the generated code, so it is pinned
    here: in every MODE >= 2 instantiation, in program order: an sc1 store, a vmcnt(0) drain, the ticket's atomic add, sc1 loads."""
    import re
    asm = _device_disassembly(tmp_path, "gcsadmm.o")
    funcs = re.split(r"\n(?=[0-9a-f]{16} <)", asm)
    seen = 0
    for f in funcs:
        m = re.match(r"[0-9a-f]{16} <(_ZN12_GLOBAL__N_111edge_kernelI[df]Li([0-3])ELi\d+ELi\d+EE[^>]*)>:", f)
        if not m:
            continue
        mode = int(m.group(2))
        lines = f.splitlines()
        idx = lambda pat, start=0: next((i for i in range(start, len(lines)) if re.search(pat, lines[i])), -1)
        if mode < 2:
            assert idx(r"global_atomic_add") < 0, m.group(1)        # no ticket outside the single-launch modes
            continue
        seen += 1
        st = idx(r"global_store_dwordx2 .* sc1")
        assert st >= 0, (m.group(1), "partials are not sc1 stores")
        wt = idx(r"s_waitcnt vmcnt\(0\)", st)
        at = idx(r"global_atomic_add", st)
        assert 0 <= wt < at, (m.group(1), "no drain between the partial stores and the ticket")
        ld = idx(r"global_load_dwordx2 .* sc1", at)
        assert ld > at, (m.group(1), "the last workgroup does not read the partials with sc1 loads")
    assert seen >= 12, seen        # {f64, f32} x {MODE 2, 3} x c in {3, 5, 7, ...}


def test_every_launching_entry_point_selects_the_handles_device():
    """Entry points work on the handle's device whatever the caller's current device is (a process may hold handles on several
    GPUs).  The structure holds that: every extern "C" function of csrc/gcsadmm.hip whose first parameter is a handle or a batch is one
    `return handle_entry(h, args, body)` / `return batch_entry(b, args, body)` -- the shim runs `args` (argument checks, on the host), takes
    the DeviceGuard and only then runs `body` -- unless it is on the named list of calls that never reach the device.  Neither those nor
    an `args` lambda may spell any device work: the guard comes before the first device call, as the earlier form of this test held."""
    import os
    import re
    from gcs_admm_amd import build
    src = open(os.path.join(build.CSRC, "gcsadmm.hip")).read()
    ext = src[src.index('extern "C" {'):]
    bodies, first_param = {}, {}
    for m in re.finditer(r"\n(?:gcsadmm_status|void|const char \*|int|int32_t) ?(gcsadmm_[a-z_0-9]+)\(([^)]*)\)\s*\n?\s*\{", ext):
        start = m.end()
        depth, i = 1, start
        while depth:
            c = ext[i]
            depth += (c == "{") - (c == "}")
            i += 1
        bodies[m.group(1)] = ext[start:i]
        first_param[m.group(1)] = m.group(2).split(",")[0]
    assert len(bodies) >= 30, sorted(bodies)
    # device work as this file spells it: the HIP runtime and kernel launches, the helpers that enqueue (launch_vertex, launch_edge, the
    # halo helpers, the partitioned loop), the owners that allocate (DevBuf upload / alloc / zero, create_owned, ensure_events,
    # overlap_setup) or release (delete h, a sub-struct of owners reset with `= {}`), RCCL, and the other objects' launch / attribute entries
    touches = re.compile(r"\bhip[A-Z]\w+\(|hipLaunchKernelGGL|\blaunch_vertex\(|\blaunch_edge\(|\bhalo_pack<|\bhalo_unpack<|\bhalo_transfer\(|\bhalo_upload\("
                         r"|\.(?:upload|alloc|zero)\(|\bcreate_owned\(|\bensure_events\(|\boverlap_setup\(|\bdelete h\b|h->(?:halo|overlap) = \{\}"
                         r"|\bset_lds_attr<|rccl\(\)\.(?!ok\b|err\b|GetErrorString\b)\w+\(|\brun_partitioned_loop\(|\bpartitioned_tail\(|gcsadmm_wg_launch|gcsadmm_wg_set")
    plain = {"gcsadmm_" + n for n in ("last_error", "batch_last_error", "query", "query_workspace", "set_fused_tail", "halo_buffers", "check_halo")}
    own_guard = {"gcsadmm_create", "gcsadmm_batch_create", "gcsadmm_destroy", "gcsadmm_batch_destroy"}      # no object yet / the owners release
    no_object = {"gcsadmm_comm_unique_id", "gcsadmm_debug_sub_cycles", "gcsadmm_debug_phase_cycles"}        # ncclGetUniqueId; symbols of the diagnostic build
    # the list must not go blind: these entry points do device work, whatever helper spells it
    must_touch = {"gcsadmm_" + n for n in ("create", "destroy", "reset", "vertex_step", "edge_step", "control", "run", "run_timed", "attach_comm",
                                           "halo_pack", "halo_unpack", "halo_exchange", "run_partitioned", "run_partitioned_timed", "set_overlap",
                                           "vertex_prox", "read_control", "cost", "unit_iterations")}
    assert must_touch | plain <= set(bodies), sorted((must_touch | plain) - set(bodies))
    assert not must_touch & plain
    shimmed = set()
    for name, body in bodies.items():
        if name in plain:
            assert not touches.search(body), f"{name} is on the list of calls that never reach the device, and touches it"
            assert not re.search(r"\b(?:handle|batch)_entry\(|DeviceGuard", body), name
            continue
        if name in own_guard:
            g = re.search(r"DeviceGuard device_guard_", body)
            assert g, f"{name} touches the device without selecting the object's device"
            early = [t.group(0) for t in touches.finditer(body[:g.start()]) if t.group(0) not in ("hipGetDeviceCount(", "hipGetErrorString(")]
            assert not early, (name, early)         # hipGetDeviceCount in create is the one query allowed before the guard
            continue
        if name in no_object:
            continue
        kind = {"gcsadmm_handle": "handle", "struct gcsadmm_batch_s *": "batch"}[re.sub(r"\w+$", "", first_param[name]).strip()]
        # one statement: `return <kind>_entry(obj, args, body)` whose closing parenthesis ends the body; before it at most declarations
        # of locals that both lambdas see (`Type name;`, nothing evaluated)
        m = re.fullmatch(rf"\s*(?:(?://[^\n]*|\w+ \w+;[^\n]*)\n\s*)*return {kind}_entry\((.*)\);\s*\}}", body, re.S)
        assert m, f"{name} is not a single `return {kind}_entry(...)`"
        depth, parts = 0, [""]
        for ch in re.sub(r'"(?:[^"\\]|\\.)*"|//[^\n]*', "", m.group(1)):
            depth += (ch in "([{") - (ch in ")]}")
            assert depth >= 0, f"{name}: the {kind}_entry call ends before the body does"
            if ch == "," and depth == 0:
                parts.append("")
            else:
                parts[-1] += ch
        assert depth == 0 and len(parts) == 3, (name, len(parts))
        # `args`, the second argument, runs BEFORE the shim takes the guard: it checks arguments on the host and nothing else
        early = [t.group(0) for t in touches.finditer(parts[1])]
        assert not early, f"{name} touches the device before the guard is taken: {early}"
        shimmed.add(name)
    assert must_touch - own_guard <= shimmed
    # the guard is taken by the shims, the creates and the destroys alone, and no entry point calls another
    for m in re.finditer(r"\bDeviceGuard \w+\(", src):
        # the last function head before it: relies on this file's layout -- a definition's head starts in column 0 on ONE line that
        # holds its name and opening parenthesis and does not end in `;`; everything inside a function is indented
        heads = re.findall(r"\n(?![ /#{}])[^\n(]*?(\w+)\([^\n]*[^;\n]\n", src[:m.start()])
        assert heads[-1] in own_guard | {"guarded_entry"}, f"a DeviceGuard in {heads[-1]}"
    for shim in ("handle_entry", "batch_entry"):
        assert re.search(rf"gcsadmm_status {shim}\([^)]*\) \{{ return guarded_entry\(", src), shim
    code = re.sub(r"//[^\n]*", "", src)
    calls = set(re.findall(r"\b(gcsadmm_[a-z_0-9]+)\(", code[code.index('extern "C" {'):])) & set(bodies)
    defs = [n for n in calls if len(re.findall(rf"\b{n}\(", code)) > 1]
    assert not defs, f"entry points called from inside gcsadmm.hip: {defs}"


def test_device_resources_are_released_by_their_owners_alone():
    """Ownership rule of the host code of the handle and of the scene (csrc/gcsadmm.hip, csrc/polytope_lp.hip with the headers split from
    them, and csrc/hip_owners.h, which has the owners): a device allocation, a stream and an event each belong to an owning type (DevBuf, Stream, Event) whose
    destructor releases it, so hipFree, hipStreamDestroy and hipEventDestroy are each written exactly once -- in the owners' releasing
    functor -- and hipMalloc only inside DevBuf.  A buffer added to the handle or the scene as a raw pointer and freed by hand fails here."""
    import os
    import re
    from gcs_admm_amd import build
    src = "".join(open(os.path.join(build.CSRC, f)).read() for f in ("hip_owners.h", "gcsadmm.hip", "loop_kernels.h", "rccl_api.h", "halo_plan.h", "polytope_lp.hip", "scene_kernels.h",
                                                                         "scene_stage.h"))
    for call in ("hipFree(", "hipStreamDestroy(", "hipEventDestroy("):
        assert src.count(call) == 1, (call, src.count(call))
    m = re.search(r"\nstruct HipRelease \{\n.*?\n\};\n", src, re.S)
    assert m, "the one releasing functor of the owners (struct HipRelease) was not found"
    assert all(call in m.group(0) for call in ("hipFree(", "hipStreamDestroy(", "hipEventDestroy("))
    m = re.search(r"\bclass DevBuf \{\n.*?\n\};\n", src, re.S)
    assert m, "the owner of device allocations (class DevBuf) was not found"
    owner = m.group(0)
    assert owner.count("hipMalloc(") >= 1
    assert len(re.findall(r"\bhip\w*Malloc\w*\(", src)) == owner.count("hipMalloc("), "an allocation outside DevBuf"
