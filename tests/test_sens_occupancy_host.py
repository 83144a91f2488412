"""CPU: every sensitivity instantiation of the built gfx950 code object — sens_kernel<MS, KIND> of csrc/nmpc_sens.hip for the plan sensitivities,
the adjoint and the forward update, and sens_dual_kernel<MS> of csrc/nmpc_sens_dual.hip, twenty each — uses no scratch and has the waves per SIMD
that its registers allow, min(8, 512 // (8 * ceil(vgpr_count / 8))), equal to WAVES below.

WAVES was filled from the code object of the commit before the three kernels of the stage recursion became one template (three kernels in three
files then), built with the same compiler and flags.  The six-robot plan kernel stands at 168 registers, the last count with three waves per
SIMD (registers are allocated in granules of 8: 136 .. 168 give three waves, 176 .. 256 two); a change to the two loops of the kernel that
crosses such an edge shows here before it shows as a slower call."""
import re

from tests import helpers as Hh

# kind -> (without, with the per-instance obstacle field), team sizes 1 .. 10
WAVES = {
    "plan":    ([5, 4, 3, 3, 3, 3, 2, 2, 2, 2], [5, 4, 3, 3, 3, 3, 2, 2, 2, 2]),
    "adjoint": ([5, 4, 3, 3, 3, 2, 2, 2, 2, 2], [5, 4, 3, 3, 3, 2, 2, 2, 2, 2]),
    "update":  ([4, 4, 3, 3, 3, 2, 2, 2, 2, 2], [5, 4, 3, 3, 3, 2, 2, 2, 2, 2]),
    "dual":    ([4, 4, 3, 3, 3, 3, 3, 3, 3, 3], [4, 4, 3, 3, 3, 3, 3, 3, 3, 3]),
}
KINDS = ["plan", "adjoint", "update"]      # KIND of sens_kernel<MS, KIND>


def waves_per_simd(vgpr_count):
    return min(8, 512 // (8 * -(-vgpr_count // 8)))


def test_no_scratch_and_the_waves_per_simd_of_the_table(built, tmp_path):
    got = {}
    for name, note in Hh.kernel_notes(tmp_path).items():
        m = re.search(r"^_ZN4nmpc11sens_kernelILi(\d+)ELi([012])EEE", name)
        d = re.search(r"^_ZN4nmpc16sens_dual_kernelILi(\d+)EEE", name)
        if not m and not d:
            assert not re.search(r"sens_\w*kernel", name), "sensitivity kernel with an unknown template signature: " + name
            continue
        kind, ms = (KINDS[int(m.group(2))], int(m.group(1))) if m else ("dual", int(d.group(1)))
        assert note["private_segment_fixed_size"] == 0, (name, note)
        got[(kind, ms // 16, ms % 16)] = waves_per_simd(note["vgpr_count"])
        print("%-8s m = %2d field %d: %3d registers, %d waves per SIMD" % (kind, ms % 16, ms // 16, note["vgpr_count"], got[(kind, ms // 16, ms % 16)]))
    want = {(kind, f, m): WAVES[kind][f][m - 1] for kind in WAVES for f in (0, 1) for m in range(1, 11)}
    assert len(want) == 80 and set(got) == set(want), (sorted(set(got) ^ set(want)))
    assert got == want, sorted((k, got[k], want[k]) for k in want if got[k] != want[k])


def test_the_formula_at_the_edges():
    assert [waves_per_simd(v) for v in (64, 65, 96, 97, 128, 129, 136, 168, 169, 176, 256, 257, 512)] == [8, 7, 5, 4, 4, 3, 3, 3, 2, 2, 2, 1, 1]
