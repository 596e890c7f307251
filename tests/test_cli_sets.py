"""The CLIs built from host/main.cpp without a GPU, one case per executable of tests/capi_testlib.CLI_SETS: `list` prints
the default dwarfs plus the executable's own set and nothing of another's, and the three places that name the sets — SETS
in host/Makefile, kDwarfSets in host/register_dwarfs.cpp, CLI_SETS — name the same ones."""
import re
import subprocess

import pytest

from tests import capi_testlib as ct
from tests.capi_testlib import CLI_SETS, DEFAULT

HOST = ct.ROOT / "dwarf_bench_amd" / "host"
PREFIX = "dwarf_bench_"


@pytest.mark.parametrize("exe", list(CLI_SETS))
def test_cli_lists_the_default_set_plus_its_own(exe):
    names = ct.cli_names(exe)
    assert names == sorted(DEFAULT + CLI_SETS[exe]), (exe, sorted(set(names) ^ set(DEFAULT + CLI_SETS[exe])))
    for other, extras in CLI_SETS.items():
        if other != exe:
            assert not set(extras) & set(names), (exe, other, sorted(set(extras) & set(names)))
    assert any(n.startswith("Slab") for n in names) == (exe == "dwarf_bench_slab"), exe
    r = subprocess.run([str(ct.LIB / exe), "NoSuchDwarf"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and f"{exe} list" in r.stderr, (exe, r.returncode, r.stderr[-300:])


def test_no_dwarf_is_in_two_sets_or_in_the_default_list():
    seen = list(DEFAULT)
    for exe, extras in CLI_SETS.items():
        for name in extras:
            assert name not in seen, (exe, name)
            seen.append(name)
    assert DEFAULT == sorted(DEFAULT) and not any(n.startswith("Slab") for n in DEFAULT)


def test_makefile_registry_and_this_table_name_the_same_sets():
    want = {exe[len(PREFIX):]: sorted(extras) for exe, extras in CLI_SETS.items() if exe != "dwarf_bench"}
    assert all(exe == "dwarf_bench" or exe.startswith(PREFIX) for exe in CLI_SETS)
    sets = re.findall(r"^SETS := (.*)$", (HOST / "Makefile").read_text(), flags=re.M)
    assert len(sets) == 1 and len(set(sets[0].split())) == len(sets[0].split()), sets
    assert sorted(sets[0].split()) == sorted(want), ("host/Makefile SETS", sorted(set(sets[0].split()) ^ set(want)))
    rows = re.findall(r'^\s*\{"(\w+)", make<(\w+)>\},', (HOST / "register_dwarfs.cpp").read_text(), flags=re.M)
    table = {}
    for name, dwarf in rows:
        owners = [s for s, dwarfs in table.items() if dwarf in dwarfs]
        assert not owners, ("host/register_dwarfs.cpp kDwarfSets", dwarf, "is in", owners + [name])
        table.setdefault(name, []).append(dwarf)
    table = {name: sorted(dwarfs) for name, dwarfs in table.items()}
    assert table == want, ("host/register_dwarfs.cpp kDwarfSets", {s: (table.get(s), want.get(s))
                                                                    for s in set(table) | set(want) if table.get(s) != want.get(s)})
