"""The engine's environment switches: one declaration (csrc/cfx_switches.h), one documentation table (DESIGN.md
section 8), and nothing else that reads or names a switch on its own.  Text only: no GPU, no library call."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cutfemx_amd" / "csrc"
HEADER = CSRC / "cfx_switches.h"

# switches that were removed: the name must not come back by accident
RETIRED = ["CFX_FACET_SORT", "CFX_ADJ_LDS", "CFX_STD_INLINE", "CFX_SCAN_PAIRS", "CFX_LAZY_ZERO", "CFX_VEC_BY_CELL",
           "CFX_DEBUG_ROWS", "CFX_C2C"]


def table_names():
    rows = re.findall(r'^\s*CFX_SWITCH\((\w+),\s*(\w+),\s*(\w+),\s*"[^"]+"\)', HEADER.read_text(), flags=re.M)
    assert rows, "no CFX_SWITCH(...) lines in the header"
    for name, kind, when in rows:
        assert kind in ("first_char", "present", "integer", "string"), (name, kind)
        assert when in ("call", "build", "once"), (name, when)
    names = ["CFX_" + r[0] for r in rows]
    assert len(set(names)) == len(names), "a switch is declared twice"
    return set(names)


def section8():
    text = (ROOT / "DESIGN.md").read_text()
    return text[text.index("## 8. Environment switches"):]


def doc_tables():
    """(engine names, python / benchmark / test names): first columns of the two tables of section 8."""
    engine, other, current = set(), set(), None
    for line in section8().splitlines():
        if line.startswith("| switch |"):
            current = engine
        elif line.startswith("| name |"):
            current = other
        elif not line.startswith("|"):
            current = None
        elif current is not None and not line.startswith("|---"):
            current.update(re.findall(r"`(CFX_[A-Z0-9_]+)", line.split("|")[1]))
    return engine, other


def test_getenv_only_in_the_switches_header():
    sites = sorted(p.name for p in CSRC.iterdir() if p.is_file() and "getenv(" in p.read_text(errors="replace"))
    assert sites == [HEADER.name], sites


def test_table_and_documentation_agree():
    engine, other = doc_tables()
    names = table_names()
    assert names - engine == set(), "declared but not documented"
    assert engine - names == set(), "documented but not declared"
    assert names & other == set()


def test_names_set_by_tests_and_tools_are_known():
    engine, other = doc_tables()
    assert engine == table_names()
    forms = [r'(?:setenv|delenv)\(\s*["\'](CFX_[A-Z0-9_]+)', r'environ\[\s*["\'](CFX_[A-Z0-9_]+)',
             r'environ\.(?:get|pop|setdefault)\(\s*["\'](CFX_[A-Z0-9_]+)', r'\benv\(\s*["\'](CFX_[A-Z0-9_]+)',
             r'["\'](CFX_[A-Z0-9_]+)["\']\s*:\s*["\']',  # {"CFX_X": "0"} handed to a child process or a helper
             r'\(\s*["\'](CFX_[A-Z0-9_]+)["\']\s*,\s*["\']']  # ("CFX_X", "0") pairs of a parametrisation
    used = {}
    for path in sorted((ROOT / "tests").glob("*.py")):
        if path.name == Path(__file__).name:
            continue
        text = path.read_text()
        for form in forms:
            for name in re.findall(form, text):
                used.setdefault(name, path.name)
    modes = (ROOT / "tools" / "test_modes.sh").read_text()
    for name in re.findall(r'"(CFX_[A-Z0-9_]+)=[^"]*"', modes):
        used.setdefault(name, "test_modes.sh")
    assert used, "the search found nothing: its patterns are broken"
    unknown = {n: f for n, f in used.items() if n not in engine and n not in other}
    assert unknown == {}, unknown


def test_retired_names_stay_retired():
    hits = []
    for top in ("cutfemx_amd", "include", "tests", "tools"):
        for path in sorted((ROOT / top).rglob("*")):
            if not path.is_file() or path.suffix in (".so", ".o", ".pyc") or path.name == Path(__file__).name:
                continue
            text = path.read_text(errors="replace")
            hits += [(str(path.relative_to(ROOT)), n) for n in RETIRED if re.search(n + r"\b", text)]
    assert hits == [], hits
    names = table_names()
    assert not names & set(RETIRED)
