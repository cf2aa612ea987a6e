"""What the COMPILER made of the backward kernel's round loop (csrc/epsm_backward_cp.hip), read off the assembly of the unit built
with the Makefile's own command plus -save-temps (tools/isa_waits.py): the rows of the scene table are requested together and
not waited for before the emission, the emission's waits leave the prefetch of the next round's record in flight, and the round
loop touches no scratch memory.  A source change that looks harmless -- a guard around a load, a first use that sinks into a
branch -- turns one trip to memory into four; the binary is the only place where that shows.  No GPU: hipcc alone."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epsm_mitsuba3_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")

# <VARIANT, DMODE = tangents in the kernel, PACKED, fixed-point rows, window, DROP>: (mangled arguments, table rows per round,
# loads of own_issue behind them)
PACKED_FORMS = {
    "manifold 2048": ("ILi0ELi2ELb1ELb0ELi2048ELb0E", 4),
    "manifold 2048, paths without a term dropped (lists)": ("ILi0ELi2ELb1ELb0ELi2048ELb1E", 4),
    "manifold 1024": ("ILi0ELi2ELb1ELb0ELi1024ELb1E", 4),
    "caustic 2048": ("ILi1ELi2ELb1ELb0ELi2048ELb1E", 3),        # no emitter row: light_grad == 0
}
OWN_ISSUE_LOADS = 9                                              # o0..o5, q6, q7, sh
ROUND_LOOP = ("round_begin", "solve", "addressing", "prefetch", "emit")


@pytest.fixture(scope="session")
def cp_assembly(tmp_path_factory):
    """The device assembly of epsm_backward_cp.hip, compiled once with the command `make` would run for its object."""
    obj = os.path.join(CSRC, "build", "epsm_backward_cp.o")
    dry = subprocess.run(["make", "-C", CSRC, "-n", "-B", "HIPCC=" + HIPCC, obj], check=True, capture_output=True, text=True).stdout
    cmd = [l for l in dry.split("\n") if "epsm_backward_cp.hip" in l and " -c " in l]
    assert len(cmd) == 1, dry
    words = cmd[0].split()
    out = tmp_path_factory.mktemp("cp_asm")
    words[words.index("-o") + 1] = str(out / "cp.o")
    subprocess.run(words + ["-save-temps"], check=True, cwd=str(out), capture_output=True, text=True)
    (s,) = [f for f in os.listdir(out) if f.endswith(".s") and "amdgcn" in f]
    return (out / s).read_text()


@pytest.mark.parametrize("form", list(PACKED_FORMS))
def test_table_rows_are_requested_together(cp_assembly, form):
    import isa_waits
    key, rows = PACKED_FORMS[form]
    s = isa_waits.summary(cp_assembly, key)
    print(form, {r: s[r] for r in ROUND_LOOP})
    assert s["addressing"]["loads"] == rows and s["addressing"]["stores"] == 0
    assert s["addressing"]["waits"] == []                       # not one of them is waited for where it is issued
    # ... and where they are (the emission), every load of the next round's record stays in flight
    assert s["emit"]["waits"] and min(s["emit"]["waits"]) >= OWN_ISSUE_LOADS


@pytest.mark.parametrize("form", list(PACKED_FORMS))
def test_round_loop_has_no_scratch_access(cp_assembly, form):
    import isa_waits
    s = isa_waits.summary(cp_assembly, PACKED_FORMS[form][0])
    assert [s[r]["scratch"] for r in ROUND_LOOP] == [0] * len(ROUND_LOOP)


def test_listing_names_every_region(cp_assembly):
    import isa_waits
    names = [r for r, _ in isa_waits.regions(cp_assembly, PACKED_FORMS["manifold 2048"][0])]
    assert names == ["prologue"] + list(ROUND_LOOP) + ["round_end"]
