"""The fused tail must not cost the workgroup program its registers (read from the compiler's resource remarks of the in-tree build, no
GPU needed): every vertex_wg_kernel instantiation keeps 0 B of scratch and 0 B of static LDS (the tail's red[4][5] and flag live in the
dynamic segment), and stays in the occupancy class it had before the tail existed."""
import re


def _kernels():
    from gcs_admm_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if "vertex_wg_kernelILi" in k}
    assert len(res) >= 40, len(res)        # n = 1 .. 8 x {f64, f32} (x BOX at n = 3, 6) x {256, 512 threads}
    return res


def test_no_scratch_no_static_lds():
    for k, v in _kernels().items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)


def test_occupancy_class_kept():
    """vector registers of the 256-thread build: n = 2, 3 at most 128 (four wavefronts per SIMD), n = 6 at most 170 (168 for the BOX
    instantiation, which runs three per SIMD: test_build.py).  512-thread build (one workgroup per CU): the classes it had before the
    tail, n = 2 at most 128, n = 3 and 6 at most 168 (three per SIMD)."""
    seen = 0
    for k, v in _kernels().items():
        n = int(re.search(r"vertex_wg_kernelILi(\d)E", k).group(1))
        regs = v["vgprs"] + v["agprs"]
        if n not in (2, 3, 6):
            continue
        seen += 1
        if "gcs_wg_t512" in k:
            assert regs <= (128 if n == 2 else 168), (k, v)
        else:
            assert regs <= (128 if n <= 3 else (168 if "Lb1E" in k else 170)), (k, v)
    assert seen == 20, seen
