"""The count-kernel variants compiled into libyawhip.so are all accounted for (no GPU needed).

The set of instantiations is read from the built library (``nm -C``: the host-side kernel handles carry the demangled
template arguments), not re-typed from the source. Every one must either be reached by a case of the GPU table of
tests/test_gpu_count_variants.py -- which asserts on the device that the library reports launching exactly those variants
and compares the results with the CPU oracle -- or be listed as unreachable there, with the reason from make_plan."""
import os
import re
import shutil
import subprocess

import pytest

import test_gpu_count_variants as table

SYMBOL = re.compile(r"::(k_count\w*<[^<>()]*>)\(")


@pytest.fixture(scope="module")
def compiled():
    from yet_another_wizz_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return {m.group(1) for line in out.splitlines() for m in SYMBOL.finditer(line)}


def test_the_library_compiles_the_count_kernel_families(compiled):
    families = {}
    for name in compiled:
        fam = name.split("<")[0]
        families[fam] = families.get(fam, 0) + 1
    assert families == {"k_count": 24, "k_count_merged": 8, "k_count_merged_occ8": 16, "k_count_band": 96, "k_count_band32": 72,
                        "k_count_band32_one": 72, "k_count_band32_fine": 32}
    assert len(compiled) == 320


def test_every_compiled_variant_is_reached_or_unreachable(compiled):
    reached = table.reached()
    unreachable = set(table.UNREACHABLE)
    assert not (reached - compiled), f"cases name variants that are not compiled: {sorted(reached - compiled)}"
    assert not (unreachable - compiled), f"unreachable variants that are not compiled: {sorted(unreachable - compiled)}"
    assert not (reached & unreachable), f"'unreachable' variants reached by a case: {sorted(reached & unreachable)}"
    missing = compiled - reached - unreachable
    assert not missing, f"{len(missing)} compiled variants have no case: {sorted(missing)[:8]}"
    assert all(table.UNREACHABLE[v] for v in unreachable)


def test_cases_are_distinct_and_each_reaches_two_launches():
    from yet_another_wizz_amd import _lib

    ids = [c.id for c in table.CASES]
    assert len(set(ids)) == len(ids)
    weighted_bit = 1 << 18
    for c in table.CASES:  # the unweighted and the weighted launch of one variant
        unweighted, weighted = (_lib.variant_code(n) for n in c.reach)
        assert unweighted & weighted_bit == 0 and weighted == unweighted | weighted_bit, c.id
    # every case reaches something no other case does: dropping one leaves compiled variants without a case
    owners = {}
    for c in table.CASES:
        for name in c.reach:
            owners.setdefault(name, []).append(c.id)
    for c in table.CASES:
        assert any(owners[name] == [c.id] for name in c.reach), c.id


def test_variant_codes_round_trip(compiled):
    from yet_another_wizz_amd import _lib

    codes = set()
    for name in compiled:
        code = _lib.variant_code(name)
        assert code > 0 and _lib.variant_name(code) == name
        codes.add(code)
    assert len(codes) == len(compiled)
    assert _lib.variant_name(_lib.VARIANT_MIXED) == "mixed"
    with pytest.raises(ValueError):
        _lib.variant_name(0)
