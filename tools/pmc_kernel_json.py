#!/usr/bin/env python
"""Per-launch averages of one kernel's counters over several rocprofv3 --pmc passes (one results.db or counter_collection.csv per pass),
as one JSON object:  python tools/pmc_kernel_json.py <kernel name> <pass output> [<pass output> ...]
The name matches a kernel exactly up to its argument list ("hs_str_group_kernel_p" does not take "hs_str_group_kernel_pw")."""
import csv
import json
import sqlite3
import sys


def _is(kernel, name):
    base = name.split("(")[0].strip().split(" ")[-1].split("::")[-1]
    return (base[:-3] if base.endswith(".kd") else base) == kernel


def _db(path, kernel, out):
    db = sqlite3.connect(path)
    n = 0
    for name, counter, avg, cnt in db.execute("select kernel_name,counter_name,avg(value),count(*) from counters_collection group by kernel_name,counter_name"):
        if _is(kernel, name):
            out[counter] = avg
            n = max(n, cnt)
    return n


def _csv(path, kernel, out):
    acc = {}
    for r in csv.DictReader(open(path)):
        if _is(kernel, r["Kernel_Name"]):
            acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    for k, v in acc.items():
        out[k] = sum(v) / len(v)
    return max((len(v) for v in acc.values()), default=0)


def main():
    kernel, out, launches = sys.argv[1], {}, []
    for p in sys.argv[2:]:
        launches.append((_csv if p.endswith(".csv") else _db)(p, kernel, out))
    if not out:
        sys.exit("no counter rows for " + kernel)
    print(json.dumps({"kernel": kernel, "launches_per_pass": launches, "per_launch": {k: out[k] for k in sorted(out)}}))


if __name__ == "__main__":
    main()
