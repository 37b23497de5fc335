"""The helper modules of tests/ stand on their own - no GPU.  Importing them (as the host-only tests and tools/ do) must not run
the body of any test module: a helper that borrows from a ``test_*`` file ties every importer to that file's fixtures, tables
and GPU set-up."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HELPERS = ("_util", "entry_points", "nonfinite_cases")


def test_helper_modules_import_no_test_module():
    code = (f"import sys; sys.path[:0] = {[os.path.join(ROOT, 'st-gcn-altformer_amd'), ROOT, HERE]!r}\n"
            f"import {', '.join(HELPERS)}\n"
            "print(*sorted(m for m in sys.modules if m.startswith('test_')))")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split() == [], f"importing {HELPERS} imported test modules: {done.stdout}"
