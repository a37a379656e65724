"""The built kernels' resources for tests/test_kernel_resources*.py, read by tools/kres.py (the
AMDGPU metadata of build/csrc/trt_kernel.o, no GPU needed): one reader of one format, shared with
the tool's listing and its --diff mode.  Whether a missing object skips or fails stays with each
test file."""
from __future__ import annotations

import importlib.util
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
OBJ = REPO / "build" / "csrc" / "trt_kernel.o"

_spec = importlib.util.spec_from_file_location("trt_tools_kres", REPO / "tools" / "kres.py")
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)


def kres(pattern: str) -> dict[str, dict[str, int]]:
    """{demangled kernel name: dict(vgpr, sgpr, scratch, lds, spill, code)} of the kernels whose
    mangled name matches the regular expression `pattern`."""
    res = {name: dict(vgpr=r["vgpr"], sgpr=r["sgpr"], scratch=r["scratch"], lds=r["lds"], spill=r["spill_v"],
                      code=r["code"]) for name, r in _tool.resources(pattern, OBJ).items()}
    assert res, f"no kernel of {OBJ} matches {pattern!r}"
    return res
