#!/usr/bin/env python3
"""Which lines and branch outcomes of the CPU oracle do the oracle-vs-reference tests execute?  CPU only, not part of the test run.

Builds oracle/libwxoracle_cov.so (gcc --coverage, -O0), runs the tests that compare the oracle with the reference's own output
(tests/test_oracle_golden.py, tests/test_oracle_sliders.py, tests/test_oracle_surface.py, tests/test_oracle_tools.py) in a child process that loads that library in place of
libwxoracle.so, then prints gcov's totals and every branch outcome never taken, with its source line.

    python tools/oracle_coverage.py [pytest arguments, default: the four test files]

A high figure says the STRUCTURE is pinned; it says nothing about the VALUES the uniforms took (that is what
the sliders64 fixtures and their sensitivity table are for)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
COV = os.path.join(ORACLE, "libwxoracle_cov.so")
CHILD = """
import sys, pytest
sys.path.insert(0, {oracle!r})
import wx_oracle
wx_oracle._LIB_PATH = {cov!r}
wx_oracle.build = lambda force=False: {cov!r}
sys.exit(pytest.main(sys.argv[1:]))
"""


def main():
    tests = sys.argv[1:] or [os.path.join(ROOT, "tests", f) for f in ("test_oracle_golden.py", "test_oracle_sliders.py", "test_oracle_surface.py", "test_oracle_tools.py")]
    for f in os.listdir(ORACLE):
        if f.endswith((".gcda", ".gcov")):
            os.remove(os.path.join(ORACLE, f))
    subprocess.check_call(["make", "-C", ORACLE, "-s", "-B", "libwxoracle_cov.so"])
    rc = subprocess.call([sys.executable, "-c", CHILD.format(oracle=ORACLE, cov=COV), "-q", "-p", "no:cacheprovider", *tests], cwd=ROOT)
    gcda = [f for f in os.listdir(ORACLE) if f.endswith(".gcda")]
    if not gcda:
        sys.exit("no .gcda written: the instrumented library was not the one loaded")
    out = subprocess.check_output(["gcov", "-b", "-c", "-o", ".", gcda[0]], cwd=ORACLE, text=True)
    blocks = [b for b in out.split("\n\n") if "wx_oracle.c'" in b.splitlines()[0:1][0]] if out.strip() else []
    print("\n".join(l for b in blocks for l in b.splitlines() if l.startswith(("File", "Lines", "Branches", "Taken"))))
    src_line, text, missed_lines, missed = 0, "", [], []
    for l in open(os.path.join(ORACLE, "wx_oracle.c.gcov")):
        m = re.match(r"\s*([^:]+):\s*(\d+):(.*)", l)
        if m:
            src_line, text = int(m.group(2)), m.group(3).strip()
            if m.group(1).strip() == "#####":
                missed_lines.append((src_line, text))
            continue
        m = re.match(r"branch\s+(\d+)\s+(never executed|taken 0)", l)
        if m:
            missed.append((src_line, int(m.group(1)), m.group(2), text))
    print(f"\nlines never executed ({len(missed_lines)}):")
    for n, t in missed_lines:
        print(f"  wx_oracle.c:{n}: {t[:110]}")
    print(f"\nbranch outcomes never taken ({len(missed)}):")
    for n, b, how, t in missed:
        print(f"  wx_oracle.c:{n} branch {b} ({how}): {t[:100]}")
    sys.exit(rc)


if __name__ == "__main__":
    main()
