"""The C-ABI library loads on a CPU-only box and exports every symbol include/yawhip.h declares.
No compute call is made here (that needs a GPU and lives in the -m gpu tests)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(yawhip_[a-z_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from yet_another_wizz_amd import _lib

    assert header_symbols() == sorted(_lib.ABI_SYMBOLS)


def test_library_exports_every_declared_symbol_at_abi_6():
    """Every declared symbol is exported, and library and header are at ABI 6 (yawhip_stats.count_variant*: the struct grew
    by two fields, so callers built against ABI 5 pass a smaller struct)."""
    from yet_another_wizz_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_symbols():
        assert hasattr(lib, name), f"libyawhip.so does not export {name}"
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    declared = int(re.search(r"#define YAWHIP_ABI_VERSION (\d+)", text).group(1))
    lib.yawhip_abi_version.restype = ctypes.c_int
    assert lib.yawhip_abi_version() == declared == 6
    assert hasattr(lib, "yawhip_count_pairs_dense_batch")


def test_errors_are_reported_not_thrown():
    from yet_another_wizz_amd import _lib

    lib = _lib.load_library()
    assert lib.yawhip_device_count(None) == -1  # YAWHIP_ERR_INVALID
    assert b"NULL" in lib.yawhip_last_error()
    if _lib.device_count() == 0:
        with pytest.raises(_lib.YawhipError, match="no HIP device|NO_DEVICE|device"):
            _lib.Context(0)


def test_stats_struct_matches_header():
    """Field order/types of the ctypes mirror follow the header's struct."""
    from yet_another_wizz_amd import _lib

    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    body = re.search(r"typedef struct yawhip_stats \{(.*?)\} yawhip_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|int32_t|double)\s+(\w+);", body)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib._Stats._fields_)


def test_dense_request_struct_matches_header():
    """The ctypes mirror of yawhip_dense_request (the record of yawhip_count_pairs_dense_batch) follows the header: same
    fields in the same order, pointers as addresses, and the C layout's size."""
    from yet_another_wizz_amd import _lib

    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    body = re.search(r"typedef struct yawhip_dense_request \{(.*?)\} yawhip_dense_request;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [n for n, _ in _lib._DenseRequest._fields_]
    assert ctypes.sizeof(_lib._DenseRequest) == 48  # two pointers, two int32, three pointers


def test_build_lists_cover_every_source_and_header(tmp_path, monkeypatch):
    """Every csrc/*.hip is compiled (the kernel units first, each on the private device header), every header is watched for staleness, and source_sha16() sees
    a change of one byte of the private header (hashed from a copy: the tree is not edited)."""
    import glob
    import shutil

    from yet_another_wizz_amd import build

    csrc = os.path.join(ROOT, "yet_another_wizz_amd", "csrc")
    assert build.KERNEL_UNITS and build.SOURCES[:len(build.KERNEL_UNITS)] == build.KERNEL_UNITS
    assert os.path.join(csrc, "yawhip.hip") in build.KERNEL_UNITS
    for unit in build.KERNEL_UNITS:
        assert '#include "yawhip_count_device.h"' in open(unit).read(), unit
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) == set(glob.glob(os.path.join(csrc, "*.hip")))
    headers = {os.path.join(ROOT, "include", "yawhip.h"), *glob.glob(os.path.join(csrc, "*.h")), *glob.glob(os.path.join(csrc, "*.inc"))}
    assert headers <= set(build.HEADERS)
    internal = os.path.join(csrc, "yawhip_internal.h")
    assert internal in build.HEADERS
    copy = str(tmp_path / "yawhip_internal.h")  # same base name: the hash covers names and contents
    shutil.copy(internal, copy)
    monkeypatch.setattr(build, "HEADERS", [copy if h == internal else h for h in build.HEADERS])
    unchanged = build.source_sha16()
    data = bytearray(open(copy, "rb").read())
    data[len(data) // 2] ^= 1
    open(copy, "wb").write(bytes(data))
    assert build.source_sha16() != unchanged
