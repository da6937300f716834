"""The C ABI of include/sdfgpu.h against the translation units of sdf_tools_amd/csrc, read from the sources (no library, no
GPU): the entry points are spread over the handle's unit, the build's and one unit per family, so every prototype must be
defined exactly once, at column 0, in some csrc/*.hip, and no sdfgpu_* function may be defined there without a prototype."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# `int sdfgpu_x(` / `const char* sdfgpu_x(` at column 0, up to whichever of `;` (a prototype) and `{` (a definition) comes first
_FUNCTION = re.compile(r"^(?:int|const char\*) (sdfgpu_\w+)\([^;{]*([;{])", re.M)


def _functions(path, end):
    return [m.group(1) for m in _FUNCTION.finditer(open(path).read()) if m.group(2) == end]


def test_every_prototype_is_defined_exactly_once_and_nothing_else_is():
    prototypes = _functions(os.path.join(ROOT, "include", "sdfgpu.h"), ";")
    assert len(prototypes) > 80 and len(set(prototypes)) == len(prototypes), "the header's prototypes were not read as expected"
    units = sorted(glob.glob(os.path.join(ROOT, "sdf_tools_amd", "csrc", "*.hip")))
    assert len(units) >= 13
    where = {}
    for unit in units:
        for name in _functions(unit, "{"):
            where.setdefault(name, []).append(os.path.basename(unit))
    missing = [n for n in prototypes if n not in where]
    twice = {n: u for n, u in where.items() if len(u) > 1}
    unlisted = {n: u for n, u in where.items() if n not in prototypes}
    assert not missing, "prototyped in include/sdfgpu.h, defined in no csrc/*.hip at column 0: %s" % missing
    assert not twice, "defined more than once: %s" % twice
    assert not unlisted, "defined in csrc/*.hip without a prototype in include/sdfgpu.h: %s" % unlisted
    # a definition that is indented (inside a namespace or a class, say) would escape the count above
    indented = re.compile(r"^[ \t]+(?:int|const char\*) (sdfgpu_\w+)\([^;{]*\{", re.M)
    for unit in units:
        assert not indented.findall(open(unit).read()), (os.path.basename(unit), indented.findall(open(unit).read()))
