"""The generated protograph tables (qldpcsim_amd/csrc/qc_tables.h,
tools/gen_qc_tables.py): the committed header is what the generator writes
today, and every table expands to exactly the bundled matrix it names."""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "qldpcsim_amd", "csrc", "qc_tables.h")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_qc_tables", os.path.join(ROOT, "tools", "gen_qc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_header_is_what_the_generator_writes(tmp_path):
    import subprocess
    import sys
    out = tmp_path / "qc_tables.h"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_qc_tables.py"), "--out", str(out)], check=True)
    assert out.read_bytes() == open(HEADER, "rb").read()


def _array(body, name):
    """Integer array `name` of one table struct of the header, nested as written."""
    txt = re.search(r"\b%s(?:\[\w+\])+ = (\{.*?\});" % name, body, re.S).group(1)
    return np.array(eval(txt.replace("{", "[").replace("}", "]")))  # digits, commas and brackets only


def test_every_table_expands_to_its_bundled_matrix():
    from qldpcsim_amd import codes
    gen = _gen()
    txt = open(HEADER).read()
    structs = re.findall(r"struct Tab(\d+) \{  // (\w+) (H[xz])\n(.*?)\n\};", txt, re.S)
    listed = re.findall(r'X\((\d+), ::qldpc::qc::Tab(\d+), "(\w+)/(H[xz])"\)', txt)
    assert structs and len(structs) == len(listed) == int(re.search(r"kNumTables = (\d+);", txt).group(1))
    assert [(i, c, h) for i, c, h, _ in structs] == [(i, c, h) for i, j, c, h in listed if i == j]
    names = {f"{c}/{h}" for _, c, h, _ in structs}
    assert {"LP118_0/Hx", "LP118_0/Hz"} <= names
    for _, code, which, body in structs:
        H = codes.load_pcm(code, which)
        dims = {k: int(v) for k, v in re.findall(r"\b(MB|NB|DC|DVMAX) = (\d+)", body)}
        cvar, cshift = _array(body, "cvar"), _array(body, "cshift")
        assert cvar.shape == cshift.shape == (dims["MB"], dims["DC"])
        assert (np.diff(cvar, axis=1) > 0).all()                      # ascending variable blocks
        assert np.array_equal(gen.expand(cvar, cshift, dims["NB"]), H)
        # the variable side lists the same edges, ascending check block per variable block
        vdeg, vchk, vslot, vshift = (_array(body, k) for k in ("vdeg", "vchk", "vslot", "vshift"))
        assert vdeg.shape == (dims["NB"],) and vchk.shape == (dims["NB"], dims["DVMAX"])
        assert int(vdeg.sum()) == cvar.size and int(vdeg.max()) == dims["DVMAX"]
        seen = set()
        for c in range(dims["NB"]):
            chk = vchk[c, :vdeg[c]]
            assert (np.diff(chk) > 0).all()
            for t in range(vdeg[c]):
                b, e = int(vchk[c, t]), int(vslot[c, t])
                assert cvar[b, e] == c and cshift[b, e] == vshift[c, t]
                seen.add((b, e))
        assert len(seen) == cvar.size


def test_report_names_the_qualifying_halves():
    tabs, report = _gen().qualifying()
    assert [(n, w) for n, w, *_ in tabs] == [("LP118_0", "Hx"), ("LP118_0", "Hz")]
    assert any(line.startswith("LP118_2/Hx") and ": no" in line for line in report)
