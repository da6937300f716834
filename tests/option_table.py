"""The option table of include/sdfgpu.h and the names sdfgpu_set_option compares against, read from the sources (no library,
no GPU): tests/test_option_table_cpu.py pins the one to the other, tests/test_gpu_options.py sets every row at its default."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# names that sdfgpu_set_option accepted until their A/B arms were removed: unknown names now
RETIRED = ("pack_variant", "ball_block", "nt_store", "y16", "march_window", "mid_threshold_y", "mid_fraction_den_y",
           "far_fraction_den_y", "far_fraction_den_x", "shell_budget_den", "fixup",
           "rows_per_chunk_y", "rows_per_chunk_x", "rows_per_chunk_zy")

_ROW = re.compile(r'^ \*  ((?:"[^"]+"(?:, )?)+)\s+\[(T|AB|U)\]\s+(-|\d+(?:(?: / |, )\d+)*)\s')


def _expand(quoted):
    """'"a/_b/_c"' -> a, a minus its last _part plus _b, ...; '"a", "b"' -> a, b."""
    names = []
    for q in re.findall(r'"([^"]+)"', quoted):
        first, *rest = q.split("/")
        names.append(first)
        names += [first[:first.rindex("_")] + r for r in rest]
    return names


def header_table():
    """[(name, tag, default)] in the header's order; default is an int, or None where the table shows '-'."""
    text = open(os.path.join(ROOT, "include", "sdfgpu.h")).read()
    text = text[text.index("/* Named integer options."):text.index("int sdfgpu_set_option(")]
    rows = []
    for line in text.splitlines():
        m = _ROW.match(line)
        if not m:
            continue
        names = _expand(m.group(1))
        defaults = [None if d == "-" else int(d) for d in re.split(r" / |, ", m.group(3))]
        if len(defaults) == 1:
            defaults *= len(names)
        assert len(defaults) == len(names), line
        rows += [(n, m.group(2), d) for n, d in zip(names, defaults)]
    return rows


def code_names():
    """The names in the if-chain of sdfgpu_set_option (sdfgpu.hip)."""
    text = open(os.path.join(ROOT, "sdf_tools_amd", "csrc", "sdfgpu.hip")).read()
    body = text[text.index("int sdfgpu_set_option("):]
    body = body[:body.index("\n}\n")]
    return re.findall(r'n == "([^"]+)"', body)
