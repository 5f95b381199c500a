"""Compile-time checks on the parts of the kernel translation unit (hipcc cross-compiles here, no GPU needed).  Every part of the
chunk pass, and the pair-table layer the household, place and contact outputs share, names what it depends on: a translation unit of esim_kernels_common.h and the part alone compiles.  And the three
diagnostics builds of csrc/Makefile (prof, prof-units, count) still compile: their macros sit inside the kernels, so they are the
first thing a change to a kernel breaks, and the product build does not see them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicsimulator_amd", "csrc")
SYNTAX = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-I", CSRC]
PARTS = ("esim_chunk_sets.h", "esim_kernels_plan.h", "esim_kernels_marks.h", "esim_kernels_draw.h", "esim_kernels_books.h", "esim_kernels_tiny.h",
         "esim_kernels_pairtab.h")


@pytest.mark.parametrize("part", PARTS)
def test_part_compiles_with_the_common_header_alone(tmp_path, part):
    tu = tmp_path / "part.hip"
    tu.write_text('#include "esim_kernels_common.h"\n#include "%s"\n' % part)
    out = subprocess.run(SYNTAX + [str(tu)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]


@pytest.mark.parametrize("defines", (("-DESIM_WAVE_PROFILE",), ("-DESIM_WAVE_PROFILE", "-DESIM_PROFILE_UNITS"), ("-DESIM_COUNT_WORK",)),
                         ids=("prof", "prof-units", "count"))
def test_diagnostics_build_compiles(defines):
    out = subprocess.run(SYNTAX + list(defines) + [os.path.join(CSRC, "esim_api.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
