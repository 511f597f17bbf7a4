#!/usr/bin/env python3
"""Summarise rocprofv3 --pmc counter_collection.csv files per kernel (mean per dispatch and sum): tools/pmc_summary.py <dir> [kernel-name regex]"""
import csv, glob, re, sys, collections
root = sys.argv[1]
pat = re.compile(sys.argv[2]) if len(sys.argv) > 2 else re.compile("conv_mfma|first_layer_rel|maxpool_rel")
data = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{root}/*/runc/*_counter_collection.csv") + glob.glob(f"{root}/*/*/*_counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        name = re.sub(r"void lrpx::|lrpx::", "", r["Kernel_Name"]); name = re.sub(r"\(.*", "", name)
        if not pat.search(name):
            continue
        data[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
cols = sorted({c for k in data.values() for c in k})
for name, cs in sorted(data.items()):
    n = max(len(v) for v in cs.values())
    print(f"\n{name}  (dispatches {n})")
    for c in cols:
        if c in cs:
            v = cs[c]
            print(f"   {c:28s} mean {sum(v)/len(v):16.1f}   sum {sum(v):18.1f}")
