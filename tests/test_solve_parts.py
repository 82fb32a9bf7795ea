"""csrc/window_solve.hip is a list of includes of csrc/solve/*.hpp, csrc/fsel.hip one of csrc/fsel/*.hpp (CPU tier: reads the include
lines, compiles nothing).

The profile guard hashes every file of those folders (scripts/solve_parts_sha256.py) and csrc/Makefile rebuilds on every one of them, whether
anything includes it or not: a part nobody includes any more would be hashed, reviewed and never compiled; a part included twice would be
compiled twice.  window_solve.hip names a part "solve/NAME.hpp"; a part that includes another one (lds.hpp: layout.hpp, schur.hpp:
schur_strip4.hpp) names it "NAME.hpp", since the compiler looks for a quoted include beside the file that includes it.
"""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anticipated-vins-mono_amd", "csrc")
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
SPLIT = pytest.mark.parametrize("top, folder", [("window_solve.hip", "solve"), ("fsel.hip", "fsel")])


def _includes_of_parts(top, folder):
    """(including file, included path) of every quoted include that lands in csrc/<folder>/ or is spelled <folder>/..."""
    parts_dir = os.path.join(CSRC, folder)
    parts = sorted(f for f in os.listdir(parts_dir) if f.endswith(".hpp"))
    found = []
    for src in [os.path.join(CSRC, top)] + [os.path.join(parts_dir, p) for p in parts]:
        for name in INCLUDE.findall(open(src).read()):
            path = os.path.normpath(os.path.join(os.path.dirname(src), name))
            if os.path.dirname(path) == parts_dir or name.startswith(folder + "/"):
                found.append((os.path.relpath(src, CSRC), path))
    return parts, found


@SPLIT
def test_every_include_of_a_solve_part_names_a_file_that_exists(top, folder):
    _, found = _includes_of_parts(top, folder)
    assert found
    missing = [(src, os.path.relpath(path, CSRC)) for src, path in found if not os.path.isfile(path)]
    assert not missing, missing


@SPLIT
def test_every_solve_part_is_included_exactly_once(top, folder):
    parts, found = _includes_of_parts(top, folder)
    assert parts
    count = {p: 0 for p in parts}
    for _, path in found:
        if os.path.dirname(path) == os.path.join(CSRC, folder) and os.path.basename(path) in count:
            count[os.path.basename(path)] += 1
    assert {p: n for p, n in count.items() if n != 1} == {}
