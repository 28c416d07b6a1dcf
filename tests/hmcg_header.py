"""What include/hmcg.h declares, parsed for the tests that hold the Python side to it (no GPU)."""
import os
import re

from hmc_jl_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmcg.h")


def extras_pointer_members():
    """The pointer members of `struct hmcg_extras`, in declaration order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+hmcg_extras\s*\{(.*?)\}\s*hmcg_extras\s*;", text, flags=re.S)
    assert body, "struct hmcg_extras not found in include/hmcg.h"
    members = [d.strip() for d in body.group(1).split(";") if d.strip()]
    ptrs = [re.search(r"(\w+)$", d).group(1) for d in members if "*" in d]
    assert len(members) == len(_lib.Extras._fields_), "include/hmcg.h and _lib.Extras disagree on the members of hmcg_extras"
    return ptrs


def _pointer(decl):
    """(name, C element type, const) of one pointer declaration."""
    m = re.fullmatch(r"(const\s+)?(\w+)\s*\*\s*(\w+)", decl.strip())
    assert m, decl
    return m.group(3), m.group(2), bool(m.group(1))


def extras_pointers():
    """{member: (C element type, const, layout)} of the pointer members of `struct hmcg_extras`; layout is the list of
    dimensions the member's comment opens with, as spelled there: `[W][ldY][K]` -> ["W", "ldY", "K"]."""
    body = re.search(r"typedef\s+struct\s+hmcg_extras\s*\{(.*?)\}\s*hmcg_extras\s*;", open(HEADER).read(), flags=re.S).group(1)
    found = {}
    for decl, dims in re.findall(r"([\w\s]+\*\s*\w+)\s*;\s*/\*\s*((?:\[[^\]]+\])+)", body):
        name, ctype, const = _pointer(decl)
        found[name] = (ctype, const, re.findall(r"\[([^\]]+)\]", dims))
    assert list(found) == extras_pointer_members(), "a pointer member of hmcg_extras without a [dim]... layout comment"
    return found


def entry_data_pointers(entry="hmcg_estimate_batch"):
    """[(name, C element type, const)] of the array parameters of an entry point, in order: every pointer parameter but
    those to the library's own structs (hmcg_config, hmcg_extras, hmcg_timing)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S)
    assert params, entry + " not found in include/hmcg.h"
    ptrs = [_pointer(d) for d in params.group(1).split(",") if "*" in d]
    return [p for p in ptrs if not p[1].startswith("hmcg_")]
