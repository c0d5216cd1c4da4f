"""Every environment switch the device library reads is either forced by a parity test or listed as diagnostic with a reason: a
new getenv("JXL_...") under jxlatte_amd/csrc/ that nobody tests fails here, without a GPU."""
import glob
import os
import re

import switch_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETENV = re.compile(r'getenv\s*\(\s*"(JXL_[A-Z0-9_]+)"')


def switches_read(src_dir):
    """names of the JXL_ variables read with getenv in the .hip / .h / .inc files of src_dir -> {name: [file, ...]}"""
    found = {}
    for pat in ("*.hip", "*.h", "*.inc"):
        for path in sorted(glob.glob(os.path.join(src_dir, pat))):
            with open(path, encoding="utf-8", errors="replace") as f:
                for name in GETENV.findall(f.read()):
                    found.setdefault(name, []).append(os.path.basename(path))
    return found


def check_inventory(src_dir):
    read = switches_read(src_dir)
    listed = set(sc.RESULT_PATH) | set(sc.DIAGNOSTIC_ONLY)
    untested = sorted(set(read) - listed)
    assert not untested, "read by the library but in neither list of tests/switch_cases.py: %s" % ", ".join(
        "%s (%s)" % (n, ", ".join(sorted(set(read[n])))) for n in untested)
    stale = sorted(listed - set(read))
    assert not stale, "listed in tests/switch_cases.py but read nowhere: %s" % ", ".join(stale)


def test_every_switch_the_library_reads_is_listed():
    read = switches_read(os.path.join(ROOT, "jxlatte_amd", "csrc"))
    assert len(read) >= 30  # (the scan finds them)
    check_inventory(os.path.join(ROOT, "jxlatte_amd", "csrc"))
    assert not set(sc.RESULT_PATH) & set(sc.DIAGNOSTIC_ONLY)
    assert all(len(reason) > 20 for reason in sc.DIAGNOSTIC_ONLY.values())


def test_a_new_getenv_is_noticed(tmp_path):
    """the scan itself: a copy of the sources with one more getenv fails the inventory, and names it"""
    import shutil
    src = os.path.join(ROOT, "jxlatte_amd", "csrc")
    dst = tmp_path / "csrc"
    shutil.copytree(src, dst)
    check_inventory(str(dst))
    with open(dst / "host.hip", "a") as f:
        f.write('\nstatic const bool jxl_foo = getenv("JXL_FOO") != nullptr;\n')
    try:
        check_inventory(str(dst))
    except AssertionError as e:
        assert "JXL_FOO (host.hip)" in str(e)
    else:
        raise AssertionError("a new getenv went unnoticed")


def test_every_result_path_switch_names_a_test_that_sets_it():
    for name, where in sc.RESULT_PATH.items():
        fname, _, test = where.partition("::")
        path = os.path.join(ROOT, "tests", fname)
        assert os.path.isfile(path), (name, where)
        with open(path, encoding="utf-8") as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(test), text, re.M), "%s: no test %s" % (name, where)
        assert re.search(r"\b%s\b" % name, text), "%s does not occur in %s" % (name, fname)


def test_every_result_path_switch_occurs_in_the_switch_tests():
    with open(os.path.join(ROOT, "tests", "test_switches_gpu.py"), encoding="utf-8") as f:
        text = f.read()
    missing = [n for n in sc.RESULT_PATH if not re.search(r"\b%s\b" % n, text)]
    assert not missing, missing


def test_every_result_path_switch_has_a_row_in_the_readme():
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        rows = [ln for ln in f.read().split("\n") if ln.startswith("|")]
    cells = " ".join(ln.split("|")[1] for ln in rows)  # first column: the variable(s) of the row
    missing = [n for n in sc.RESULT_PATH if not re.search(r"`%s\b" % n, cells)]
    assert not missing, missing
