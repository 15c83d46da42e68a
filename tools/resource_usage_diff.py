"""Compare two build logs made with EXTRA=-Rpass-analysis=kernel-resource-usage
(make -C qldpcsim_amd/csrc EXTRA=... 2> log): prints one line per kernel of the
second log, 'same' where every resource line equals the first log's, 'CHANGED'
with both where not, 'new' for a kernel the first log does not have (the
format of profiles/*/resource_usage.txt).

  python tools/resource_usage_diff.py parent.log branch.log [substring]

With a substring only kernels whose demangled name holds it are printed; the
exit status is 1 if any kernel of the first log changed or disappeared."""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("SGPRs Spill", "sgpr-spill"),
          ("VGPRs Spill", "vgpr-spill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "waves/SIMD"), ("LDS Size [bytes/block]", "static-LDS"))


def parse(path):
    """{mangled name: {field: value}} in the log's order (a kernel compiled
    more than once, e.g. per translation unit, keeps its last record)."""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    short = [re.sub(r"\(.*$", "", s) for s in r.stdout.splitlines()]
    return dict(zip(names, short))


def fmt(rec):
    return " ".join(f"{label} {rec.get(key, '?')}" for key, label in FIELDS)


def main(argv):
    old, new = parse(argv[1]), parse(argv[2])
    only = argv[3] if len(argv) > 3 else ""
    names = demangle(list(dict.fromkeys(list(new) + list(old))))
    bad = 0
    for k, rec in new.items():
        if only not in names[k]:
            continue
        if k not in old:
            print(f"new      {names[k]}  {fmt(rec)}")
        elif fmt(old[k]) == fmt(rec):
            print(f"same     {names[k]}  {fmt(rec)}")
        else:
            bad += 1
            print(f"CHANGED  {names[k]}  {fmt(old[k])}  ->  {fmt(rec)}")
    for k in old:
        if k not in new and only in names[k]:
            bad += 1
            print(f"GONE     {names[k]}  {fmt(old[k])}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
