"""CPU-only checks of the C ABI: the library builds, loads, and exports every symbol that
include/wmf_hip.h declares; argument validation that needs no GPU; ctypes table in sync."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "wmf_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from recmodel_amd import _lib
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wmf_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(lib):
    names = declared_symbols()
    assert len(names) >= 18
    for name in names:
        assert hasattr(lib, name), f"{name} declared in wmf_hip.h but not exported by libwmf_hip.so"


def test_ctypes_table_matches_header(lib):
    from recmodel_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wmf_hip.h"\nint main(void){ return WMF_OK + (int)sizeof(int64_t) - 8; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_header_cites_reference_lines():
    text = open(HEADER).read()
    for cite in ("wmf_model.py:213-240", "wmf_model.py:311-351", "base_model.py:150-179", "wmf_model.py:191-211"):
        assert cite in text


def test_pure_host_entry_points(lib):
    assert lib.wmf_version() >= 100
    assert [lib.wmf_ld_for(f) for f in (1, 16, 64, 65, 129, 257)] == [4, 16, 64, 68, 132, 260]
    assert lib.wmf_gram_workspace_bytes(64) > 0 and lib.wmf_gram_workspace_bytes(0) == 0
    assert lib.wmf_eval_workspace_bytes() > 0
    assert lib.wmf_profile_reset() == 0 and lib.wmf_profile_collect() == 0       # nothing recorded: an empty table
    assert lib.wmf_profile_entry(0, None, 0, None, None, None, None, None) == -1  # WMF_EINVAL, no entry 0
    assert lib.wmf_debug_set_flags(2) == -1                                      # ablation switches: -DWMF_LAB builds only
    assert lib.wmf_debug_set_flags(0) == 0
    # the split layout of the whitened fixed side (k = 16 m with biases, m + 1 not a multiple of 4): the same predicate in
    # the library and in the CPU stand-in the host-logic tests run on
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fake_kernels import NumpyKernels
    fk = NumpyKernels()
    for f in list(range(1, 150)) + [161, 193, 257]:
        ld = lib.wmf_ld_for(f)
        for bias in (0, 1):
            assert lib.wmf_whitened_row_floats(f, ld, bias) == fk.whitened_row_floats(f, ld, bool(bias)), (f, bias)
    assert [lib.wmf_whitened_row_floats(f, lib.wmf_ld_for(f), 1) for f in (17, 33, 49, 65, 113, 129, 145)] == [16, 32, 52, 64, 116, 128, 148]
    assert lib.wmf_whitened_row_floats(129, 132, 0) == 132


def test_float64_workspace_layout_is_unchanged(lib):
    """wmf_half_step_f64_workspace_bytes is host arithmetic over the one layout that wmf_launch_half_step_f64 carves as well
    (F64Workspace, csrc/wmf_f64.hip).  The table was recorded from the library before that layout was written once: the sum of
    its aligned parts must not move."""
    shapes = ((0, 0), (1, 1), (1000, 37), (100003, 250001))
    recorded = {
        1: [6144, 6656, 15360, 4856320],
        16: [567552, 568064, 704256, 47867392],
        17: [642048, 642560, 789248, 50991616],
        65: [8952320, 8953344, 9550336, 200591872],
        129: [34970624, 34972160, 36255744, 426179072],
        144: [43513088, 43514624, 44962560, 481963520],
        145: [44142592, 44144128, 45614848, 487240192],
        257: [138223616, 138226176, 141177856, 966908416],
    }
    for f, want in recorded.items():
        assert [lib.wmf_half_step_f64_workspace_bytes(f, m, n) for m, n in shapes] == want, f


CSRC = os.path.join(ROOT, "recmodel_amd", "csrc")


def header_debug_flags():
    """{name: (value, lab only)} of the WMF_DBG_* enum of include/wmf_hip.h: one constant per line, `lab` the first word of its comment."""
    rows = re.findall(r"^\s*(WMF_DBG_\w+)\s*=\s*(\d+),?\s*/\*\s*(lab\b)?", open(HEADER).read(), flags=re.M)
    assert len(rows) == len({name for name, _, _ in rows})
    return {name: (int(value), bool(lab)) for name, value, lab in rows}


def test_debug_flag_table_is_one_table():
    """The header's enum, the dict of recmodel_amd/_lib.py and the mask the shipped library accepts (wmf_internal.h) name the
    same switches; every one is a single bit; every switch the shipped library accepts is set by a GPU test."""
    import glob
    from recmodel_amd import _lib
    table = header_debug_flags()
    assert len(table) >= 21
    assert {name: value for name, (value, _) in table.items()} == _lib.DEBUG_FLAGS
    assert all(value & (value - 1) == 0 for value in _lib.DEBUG_FLAGS.values())
    assert len(set(_lib.DEBUG_FLAGS.values())) == len(_lib.DEBUG_FLAGS) and 512 not in _lib.DEBUG_FLAGS.values()
    shipped = sorted(name for name, (_, lab) in table.items() if not lab)
    assert shipped == sorted(_lib.SHIPPED_DEBUG_FLAGS) and len(shipped) == 6
    internal = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "wmf_internal.h")).read())
    masks = {m.group(1): sorted(re.findall(r"WMF_DBG_\w+", m.group(2)))
             for m in re.finditer(r"constexpr int (WMF_DBG_SHIPPED|WMF_DBG_LAB) =([^;]*);", internal)}
    assert masks["WMF_DBG_SHIPPED"] == shipped
    assert masks["WMF_DBG_LAB"] == sorted(name for name, (_, lab) in table.items() if lab)
    gpu_tests = "".join(open(path).read() for path in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    for name in shipped:
        assert re.search(r"\b%s\b" % name, gpu_tests), f"{name} is accepted by the shipped library, but no tests/test_gpu_*.py sets it"


def test_no_magic_switch_numbers_in_csrc():
    """No decimal literal is tested against the switches any more: the names of include/wmf_hip.h only."""
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        for pattern in (r"(wmf_debug_flags|dbg)\s*&\s*\(?\s*~?\s*\d", r"WMF_ABL\(\w+,\s*\d"):
            found = re.search(pattern, text)
            assert not found, f"{fn}: {found.group(0)!r}"


def test_shipped_library_accepts_the_tested_switches_only(lib):
    from recmodel_amd import _lib
    assert os.path.basename(_lib.LIB_PATH) == "libwmf_hip.so"                    # (not a lab build selected by WMF_HIP_LIB)
    try:
        for name, value in _lib.DEBUG_FLAGS.items():
            if name in _lib.SHIPPED_DEBUG_FLAGS:
                assert lib.wmf_debug_set_flags(value) == 0, name
                assert lib.wmf_debug_get_flags() == value
            else:
                before = lib.wmf_debug_get_flags()
                assert lib.wmf_debug_set_flags(value) == _lib.WMF_EINVAL, name
                assert lib.wmf_debug_set_flags(value | _lib.DEBUG_FLAGS["WMF_DBG_NO_ITER"]) == _lib.WMF_EINVAL, name
                assert lib.wmf_debug_get_flags() == before                        # a refused call changes nothing
        for value in (512, 4, 16, 32, 128, 16384, 1 << 20, -1):                  # 512: reserved; the others were never switches
            assert lib.wmf_debug_set_flags(value) == _lib.WMF_EINVAL, value
        everything = sum(_lib.DEBUG_FLAGS[name] for name in _lib.SHIPPED_DEBUG_FLAGS)
        assert lib.wmf_debug_set_flags(everything) == 0 and lib.wmf_debug_get_flags() == everything
    finally:
        assert lib.wmf_debug_set_flags(0) == 0
    assert lib.wmf_debug_get_flags() == 0


def test_debug_flag_names_parse():
    from recmodel_amd import _lib
    assert _lib.parse_debug_flags("268435456") == _lib.parse_debug_flags("WMF_DBG_NO_ITER") == _lib.parse_debug_flags("NO_ITER") == 268435456
    assert _lib.parse_debug_flags("NO_ITER|F64_VALU") == 268435456 | 536870912
    assert _lib.parse_debug_flags("0x1000 | 131072") == 4096 | 131072 and _lib.parse_debug_flags("0") == 0
    with pytest.raises(ValueError):
        _lib.parse_debug_flags("NO_SUCH_SWITCH")


def test_shipped_library_reads_no_environment(lib):
    """The policy of the matrix-free iteration (csrc/wmf_iter.hip) is compiled in: the shipped library does not import getenv."""
    from recmodel_amd import _lib
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    symbols = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert "hipLaunchKernel" in symbols or any(s.startswith("hip") for s in symbols)   # (the listing is not empty)
    assert "getenv" not in symbols and "secure_getenv" not in symbols


def test_iter_on_follows_the_switch(lib):
    """AlsEngine.iter_on, which the benchmark's byte model reads, is the library's switch and not a constant."""
    from recmodel_amd import _lib
    from recmodel_amd.engine import AlsEngine
    assert isinstance(AlsEngine.__dict__["iter_on"], property)
    read = AlsEngine.__dict__["iter_on"].fget
    try:
        assert read(None) is True
        assert lib.wmf_debug_set_flags(_lib.DEBUG_FLAGS["WMF_DBG_NO_ITER"]) == 0
        assert read(None) is False
    finally:
        lib.wmf_debug_set_flags(0)


def test_argument_validation_without_gpu(lib):
    from recmodel_amd import _lib
    dummy = ctypes.c_void_p(16)
    # ld not a multiple of 4 / smaller than f -> WMF_EINVAL -> ValueError, before any HIP call
    with pytest.raises(ValueError):
        _lib.check(lib.wmf_gram(dummy, 10, 64, 63, 0, dummy, dummy, None))
    with pytest.raises(ValueError):
        _lib.check(lib.wmf_row_transform(dummy, 10, 300, 300, dummy, 0, dummy, None, None))
    with pytest.raises(ValueError):   # the reference's predict() length rule (wmf_model.py:200-203)
        _lib.check(lib.wmf_predict_pairs(dummy, dummy, 16, 16, 0, dummy, 3, dummy, 2, dummy, None))
    with pytest.raises(ValueError):
        _lib.check(lib.wmf_confidence_transform(dummy, 5, 10.0, 1.0, 7, None))
    bad_ptr = np.array([0, 2, 1], dtype=np.int64)   # not monotone
    plan = ctypes.c_void_p()
    with pytest.raises(ValueError):
        _lib.check(lib.wmf_plan_create(bad_ptr.ctypes.data_as(ctypes.c_void_p), 2, 16, 0, ctypes.byref(plan)))


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import scipy.sparse as sp
    from recmodel_amd import WMF, _lib
    m = WMF(num_items=5, num_users=4, dim=2, gamma=0.1, weighted=True)
    c = sp.random(4, 5, density=0.5, format="csr", random_state=0)
    with pytest.raises(_lib.WmfLibraryError):
        m.train(utility_mat=c, iterations=1, eval_mat=c, count_mat=c)
    with pytest.raises(_lib.WmfLibraryError):
        m.recompute_factors(m.items, c, 0.1)


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, "recmodel_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in text.replace("test infrastructure", ""), f"{fn} mentions the oracle"


def test_lds_dma_kernel_leaves_in_flight_registers_alone():
    """wmf_directl.hip reads its LDS ring with inline-asm ds_reads whose destination registers hipcc believes written at
    once; nothing may touch them before the inline-asm wait that retires them (tools/check_inflight_regs.py parses the
    gfx950 assembly of the file -- no GPU needed)."""
    import subprocess
    import sys
    script = os.path.join(ROOT, "tools", "check_inflight_regs.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 violations" in res.stdout


def test_iteration_kernel_leaves_in_flight_registers_alone():
    """wmf_iter.hip (the default k = 128 path since round 4) reads LDS through inline-asm ds_reads too: the same scan of its
    gfx950 assembly, and it must have found the reads it is there to check."""
    import re
    import subprocess
    import sys
    script = os.path.join(ROOT, "tools", "check_inflight_regs.py")
    src = os.path.join(ROOT, "recmodel_amd", "csrc", "wmf_iter.hip")
    res = subprocess.run([sys.executable, script, src], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 violations" in res.stdout
    assert int(re.search(r"(\d+) inline-asm ds_reads checked", res.stdout).group(1)) > 0

