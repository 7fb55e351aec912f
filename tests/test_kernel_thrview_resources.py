"""Resources of the threshold view's kernel (csrc/thrview.hip), read from the built library's gfx950 code objects (no GPU
needed): no scratch memory, no spilled vector or scalar register -- a byte-wise form of the 16-pixel step once took every
vector register and spilled 600 scalar ones, unnoticed by any output test --, no LDS, and registers that fit its launch
bounds with room to spare: 256 threads are one wave per SIMD, and at 128 vector registers or fewer four such workgroups
share a compute unit.  Only these metadata fields are looked at."""
import test_kernel_view_resources as R

KERNEL = "k_thrview"


def test_the_threshold_view_kernel_needs_no_scratch_no_lds_and_fits_its_launch_bounds(tmp_path, monkeypatch):
    monkeypatch.setattr(R, "KERNELS", (KERNEL,))          # (thrview.hip's anonymous namespace mangles as view.hip's)
    found = R._blocks(tmp_path)
    assert sorted(found) == [KERNEL], "k_thrview is missing from the gfx950 code objects"
    assert len(found[KERNEL]) == 1
    block = found[KERNEL][0]
    for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"):
        assert R._field(block, field, KERNEL) == 0, f"{field} = {R._field(block, field, KERNEL)}"
    assert R._field(block, "max_flat_workgroup_size", KERNEL) == 256
    assert R._field(block, "wavefront_size", KERNEL) == 64
    assert R._field(block, "vgpr_count", KERNEL) <= 128, f"{R._field(block, 'vgpr_count', KERNEL)} VGPRs"
