#!/usr/bin/env python3
"""make_encoder_cases.py — golden for tests/test_encoder_cases_cpu.py and tests/test_gpu_encoder_cases.py.

    python tests/golden/make_encoder_cases.py <reference checkout>

Runs the input of every case of tests/_encoder_cases.py through the REFERENCE's deflate() (bundle dist/cjs/zlib.js under
Node) and writes encoder_cases.json: per case the input's length and sha256, the length and sha256 of what the reference
made, and the census (the rules the oracle's tokens and headers show on the input).  Only those numbers and names are
committed: no input bytes, nothing of the reference.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402  (the generators live in the C-ABI library)
import _encoder_cases as ec  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
bundle = os.path.join(sys.argv[1], "dist", "cjs", "zlib.js")
cases = ec.cases(ge.load())
js = (
    "const Z=require(process.argv[1]);const fs=require('fs');const crypto=require('crypto');"
    "const out=process.argv.slice(2).map(p=>{const d=Buffer.from(Z.deflate(new Uint8Array(fs.readFileSync(p))));"
    "return {len:d.length,sha:crypto.createHash('sha256').update(d).digest('hex')};});"
    "console.log(JSON.stringify(out));"
)
names = sorted(cases)
with tempfile.TemporaryDirectory() as td:
    paths = []
    for i, name in enumerate(names):
        paths.append(os.path.join(td, "%03d.bin" % i))
        cases[name].data.tofile(paths[-1])
    res = json.loads(subprocess.check_output(["node", "-e", js, bundle] + paths, timeout=1800))
out = {}
for name, r in zip(names, res):
    k = cases[name]
    out[name] = {"n": int(k.data.size), "input_sha256": hashlib.sha256(k.data.tobytes()).hexdigest(), "deflate_len": r["len"],
                 "deflate_sha256": r["sha"], "census": ec.census(k.data, k.deep)}
with open(os.path.join(HERE, "encoder_cases.json"), "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print("encoder_cases.json: %d cases" % len(out))
