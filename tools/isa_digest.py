#!/usr/bin/env python3
"""Per-kernel digest of the device code of a csrc directory:  tools/isa_digest.py materialrefgs_amd/csrc [stem ...]

A diff aid for refactors: run it on two checkouts and diff the output.  For every .hip file it asks `make -n -B <stem>.o` for the
compile line (so it holds no flag table and works with any Makefile that has such a rule), reruns that line with
--cuda-device-only -S and prints, per kernel:  file  name  instruction lines  hash  vgpr  sgpr  scratch bytes  LDS bytes.
Before hashing, only comments, the function index in .LBB<n>_<m> labels and the symbol names in @rel32 references are normalised.
"""
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def device_asm(csrc, stem):
    dry = subprocess.run(["make", "-n", "-B", stem + ".o"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    line = next(l for l in dry.splitlines() if f"-c {stem}.hip" in l)
    argv = shlex.split(line)
    o = argv.index("-o")
    del argv[o:o + 2]
    argv[argv.index("-c"):argv.index("-c") + 1] = ["--cuda-device-only", "-S"]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, stem + ".s")
        subprocess.run(argv + ["-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def digest(csrc, stem):
    asm = device_asm(csrc, stem)
    meta = {}  # kernel name -> the four resource numbers, from the amdhsa.kernels metadata
    for entry in re.split(r"\n  - ", asm[asm.find("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            meta[name.group(1)] = [re.search(rf"\.{k}:\s+(\d+)", entry).group(1) for k in META]
    rows = []
    for name, res in meta.items():
        body = asm[asm.index(f"\n{name}:") + 1:]
        body = body[:body.index("\n.Lfunc_end")]
        lines, count = [], 0
        for l in body.splitlines()[1:]:
            l = l.split(";")[0].strip()
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            l = re.sub(r"[\w.$]+@rel32", "SYM@rel32", l)
            if not l or (l.startswith(".") and not l.startswith(".LBB")):
                continue
            lines.append(l)
            count += not l.endswith(":")
        h = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
        rows.append(f"{stem:20s} {name:90s} {count:6d} {h} " + " ".join(f"{r:>5s}" for r in res))
    return sorted(rows)


def main():
    csrc = sys.argv[1]
    stems = sys.argv[2:] or sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for rows in pool.map(lambda s: digest(csrc, s), stems):
            print("\n".join(rows))


if __name__ == "__main__":
    main()
