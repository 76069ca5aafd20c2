"""Kernel texts (`emme_amd/csrc/*_text.hpp`): files that are read, with selector macros set,
by one or more kernel units.  The build has to know about them: a text that the Makefile's HDRS does not list can be
edited without its units being rebuilt, and a reader outside SRCS is never compiled.  Reads sources only.  No GPU."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "emme_amd" / "csrc"
TEXTS = sorted(p.name for p in CSRC.glob("*_text.hpp"))


def _makefile_list(name):
    """The words of `name = ...` in the Makefile, continuation lines joined."""
    text = (CSRC / "Makefile").read_text().replace("\\\n", " ")
    m = re.search(r"^%s\s*=(.*)$" % re.escape(name), text, re.M)
    assert m, name
    return m.group(1).split()


def _code_lines(path):
    """Lines of a source file outside // comments (the texts use no block comments)."""
    return [line.split("//")[0] for line in path.read_text().splitlines()]


# the six thin units of the table-free tile fill: each is one reading of assemble_tile_text.hpp
TILE_UNITS = ["assemble_tile.hip", "assemble_tile_deriv.hip", "assemble_tile_sets.hip", "assemble_tile_sets_deriv.hip",
              "assemble_tile_shape.hip", "assemble_tile_shape_deriv.hip"]
TILE_SELECTORS = {"EMME_TILE_SHAPE", "EMME_TILE_SETS", "EMME_TILE_DERIV"}
# the two units of the cached derivative fill and the reading of assemble_dense_deriv_text.hpp that each is
DENSE_DERIV_UNITS = {"assemble_dense_deriv.hip": "0", "assemble_dense_shape_deriv.hip": "1"}


def test_there_are_texts():
    assert TEXTS == ["assemble_dense_deriv_text.hpp", "assemble_deriv_list_text.hpp", "assemble_nodes_text.hpp",
                     "assemble_sets_list_text.hpp", "assemble_tile_text.hpp", "assemble_wl_text.hpp"], TEXTS


def test_every_tile_unit_defines_the_three_selectors():
    """Exactly the text's three selectors, each once and to 0 or 1, before the unit reads the text."""
    for u in TILE_UNITS:
        lines = _code_lines(CSRC / u)
        inc = next(k for k, line in enumerate(lines) if re.match(r'\s*#\s*include\s+"assemble_tile_text\.hpp"', line))
        defs = [m.group(1) for line in lines[:inc] for m in [re.match(r"\s*#\s*define\s+(\w+)\s+[01]\s*$", line)] if m]
        assert sorted(defs) == sorted(TILE_SELECTORS), (u, defs)
        assert not any(re.match(r"\s*#\s*define\s+EMME_TILE_", line) for line in lines[inc:]), u


def test_both_dense_deriv_units_define_the_selector():
    """The text's one selector, once, to the unit's own value, before the unit reads the text; none after it."""
    for u, value in DENSE_DERIV_UNITS.items():
        lines = _code_lines(CSRC / u)
        inc = next(k for k, line in enumerate(lines)
                   if re.match(r'\s*#\s*include\s+"assemble_dense_deriv_text\.hpp"', line))
        defs = [m.groups() for line in lines[:inc]
                for m in [re.match(r"\s*#\s*define\s+(EMME_DENSE_DERIV_\w+)\s+(\S+)\s*$", line)] if m]
        assert defs == [("EMME_DENSE_DERIV_SHAPE", value)], (u, defs)
        assert not any(re.match(r"\s*#\s*define\s+EMME_DENSE_DERIV_", line) for line in lines[inc:]), u


def test_every_text_is_a_makefile_header():
    hdrs = _makefile_list("HDRS")
    for t in TEXTS:
        assert t in hdrs, "%s is not in the Makefile's HDRS: editing it would not rebuild its units" % t


def test_every_text_refuses_an_undefined_selector():
    for t in TEXTS:
        lines = [line.strip() for line in _code_lines(CSRC / t) if line.strip()]
        # the first directives of the text: an #if(n)def / #if !defined on the selector, then #error
        first = next(k for k, line in enumerate(lines) if line.startswith("#"))
        assert re.match(r"#\s*(ifndef\s+EMME_\w+|if\s+!defined\(EMME_\w+\))", lines[first]), (t, lines[first])
        assert lines[first + 1].startswith("#error"), (t, lines[first + 1])
        # and every selector the text branches on is covered by that guard
        guarded = set(re.findall(r"EMME_\w+", lines[first]))
        used = set()
        for line in lines:
            if re.match(r"#\s*(if|elif)\b", line):  # (#ifndef of an overridable default is no selector)
                used |= set(re.findall(r"EMME_\w+", line))
        assert used and used <= guarded, (t, sorted(used - guarded))


def test_every_reader_of_a_text_is_compiled():
    srcs = set(_makefile_list("SRCS"))
    readers = {}
    for path in sorted(CSRC.iterdir()):
        if path.suffix not in (".hip", ".cpp", ".hpp", ".h"):
            continue
        for line in _code_lines(path):
            m = re.match(r'\s*#\s*include\s+"(\w+_text\.hpp)"', line)
            if m:
                readers.setdefault(m.group(1), set()).add(path.name)
    for t in TEXTS:
        assert readers.get(t), "%s is read by nobody" % t
        for r in readers[t]:
            assert r in srcs, "%s reads %s but is not in the Makefile's SRCS" % (r, t)
