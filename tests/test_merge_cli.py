"""CPU: the `fermi-amd` usage banner names the index-merging commands (host/main.c)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def test_usage_lists_merge_and_recode():
    if not os.path.exists(AMD):
        pytest.skip("fermi-amd is not built here")
    p = subprocess.run([AMD], capture_output=True, timeout=60)
    assert p.returncode == 1
    err = p.stderr.decode()
    assert "merge      merge FMD-indexes (fermi merge)" in err
    assert "recode     RLE\\6 -> RLD\\2 (fermi recode)" in err
