import atexit
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# MIOpen adds what its searches find to the user database the package points it at: the tuned, committed files under
# sejonggo_amd/miopen_db.  The suite (and every process it starts) works on a copy of them, so a test run leaves the
# tree as it found it.
if "MIOPEN_USER_DB_PATH" not in os.environ:
    _db = tempfile.mkdtemp(prefix="sgo_miopen_db_")
    _src = os.path.join(ROOT, "sejonggo_amd", "miopen_db")
    for _f in os.listdir(_src) if os.path.isdir(_src) else []:
        if _f.endswith(".txt"):
            shutil.copy2(os.path.join(_src, _f), _db)
    os.environ["MIOPEN_USER_DB_PATH"] = _db
    atexit.register(shutil.rmtree, _db, True)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
