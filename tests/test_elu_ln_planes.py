"""mms_elu_ln_planes16_group (include/mms.h) entry by entry (tests/elu_ln_planes_check.py) on the CPU build of the C ABI.
tests/test_elu_ln_planes_gpu.py runs the same list on the HIP build."""
import os
import subprocess

import pytest

import elu_ln_check as ec
import elu_ln_planes_check as pc
from massive_marl_benchmark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu():
    return _lib.lib_cpu(), -1, None, "cpu"


def test_abi_declares_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "#define MMS_ABI_VERSION 4" in hdr and _lib.lib_cpu().mms_abi_version() == 4            # an addition: the version stays
    assert "int %s(" % pc.NEW in hdr and pc.NEW in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.LIB_CPU_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert " T %s\n" % pc.NEW in out, path


@pytest.mark.parametrize("H,M", ec.SHAPES)
def test_equals_the_composition(H, M):
    pc.check_composition(*_cpu(), H, M)


def test_equals_the_composition_at_the_widest_row():
    pc.check_composition(*_cpu(), *ec.BIG, G=1)


def test_equals_the_composition_32_networks():
    pc.check_composition(*_cpu(), 36, 7, G=32)


def test_zero_rows_and_a_bound_at_a_power_of_two():
    pc.check_adversarial_rows(*_cpu())


@pytest.mark.parametrize("H", [100, 64, 512])
def test_rows_independent_and_deterministic(H):
    pc.check_rows_independent(*_cpu(), H)


def test_no_rows_and_null_scale_entries():
    pc.check_empty_and_null_entries(*_cpu())


def test_contract():
    pc.check_contract(*_cpu())


def test_kernels_keep_no_scratch():
    """The built HIP library's gfx950 code objects, read as test_host_logic.py::test_kernel_resources_of_the_built_library reads them:
    elu_ln_planes_kernel has no scratch and, like elu_ln_kernel, stays at or under 128 VGPRs (no bound on its occupancy: a streaming
    pass of 256-thread workgroups; four waves per SIMD are what 128 registers leave)."""
    import re
    import struct
    import tempfile
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    data = open(_lib.LIB_PATH, "rb").read()
    kernels, pos = {}, 0
    while True:                                                     # one offload bundle per object file of the library
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", pos)
        if i < 0:
            break
        pos = i + 24
        n = struct.unpack_from("<Q", data, i + 24)[0]
        off, code = i + 32, None
        for _ in range(n):
            o, s, tl = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + tl].decode()
            off += tl
            if "gfx950" in triple:
                code = data[i + o:i + o + s]
        if not code or b"elu_ln_planes_kernel" not in code:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(code)
            f.flush()
            notes = subprocess.check_output([readelf, "--notes", f.name]).decode()
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(_Z\S+)", block).group(1)
            kernels[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    fwd = {k: v for k, v in kernels.items() if "elu_ln_kernel" in k or "elu_ln_planes_kernel" in k}
    print(fwd)
    assert len(fwd) == 2, sorted(kernels)
    for k, (vgpr, scratch) in fwd.items():
        assert scratch == 0 and vgpr <= 128, (k, vgpr, scratch)
