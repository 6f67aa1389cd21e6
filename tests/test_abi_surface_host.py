"""The dynamic symbol table of libdrt_hip.so is the C ABI and nothing else of the host layer: the functions include/drt_hip.h declares are
exported, every one of them, and no internal helper of the host units (csrc/drt_capi*.cpp, drt_host.h) is.  Before the host layer was split
into units, `check_px` and `pixel_dist_film` - anonymous namespaces opened inside an `extern "C"` block - and `DevBuf::resize` were.

The kernel units' own C++ symbols (drt::launch_*, the kernels' stubs) are mangled or begin with an underscore and are not this test's
business.  No device is needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    """Names of the functions include/drt_hip.h declares: `drt_<name>(` outside comments."""
    text = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"\b(drt_[A-Za-z0-9_]+)\s*\(", text))


def _exported(path):
    """(name, type letter) of the defined dynamic symbols (nm -D --defined-only)."""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = []
    for line in out.splitlines():
        parts = line.split()
        if len(parts) >= 2:
            syms.append((parts[-1].split("@")[0], parts[-2]))
    return syms


@pytest.mark.parametrize("hooks", [False, True], ids=["production", "hooks"])
def test_library_exports_the_header_and_no_host_internals(uivr, hooks):
    from uivr_amd._native import library_path
    path = library_path(hooks)
    if hooks and not os.path.exists(path):
        pytest.skip("the test-hooks flavour is not built")
    declared = _declared()
    assert len(declared) >= 88, "the header's declarations were not found"
    syms = _exported(path)
    functions = {n for n, t in syms if t in "TtWwi"}
    drt = {n for n in functions if n.startswith("drt_")}
    assert drt == declared, f"only declared: {sorted(declared - drt)}; only exported: {sorted(drt - declared)}"
    # unmangled, no leading underscore, not drt_*: a helper that got C linkage by accident (the check_px / pixel_dist_film leak)
    stray = sorted(n for n in functions if not n.startswith("_") and n not in declared)
    assert not stray, f"{os.path.basename(path)} exports internal helpers: {stray}"
    # ... and the host units' C++ internals stay hidden: namespace drt::host, anything of or over the handle (the DevBuf::resize leak)
    internal = sorted(n for n, _ in syms if "DevBuf" in n or "3drt4host" in n or "12drt_handle_s" in n)
    assert not internal, f"{os.path.basename(path)} exports host-layer internals: {internal}"
