#!/usr/bin/env python3
"""make_live_reference.py — golden for test_oracle_matches_live_reference (tests/test_oracle_golden.py).

    python tests/golden/make_live_reference.py <reference checkout>

Runs the test's random inputs through the REFERENCE's deflate() (bundle dist/cjs/zlib.js under Node) and writes
live_reference.json: per input its length and sha256, and either the length + sha256 of what the reference made or
the message it threw.  Only those numbers are committed.
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
import __graft_entry__ as ge  # noqa: E402  (the generators live in the C-ABI library: zes_gen.c)
from test_oracle_golden import live_reference_inputs  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
bundle = os.path.join(sys.argv[1], "dist", "cjs", "zlib.js")
inputs = live_reference_inputs(ge.load())
js = (
    "const Z=require(process.argv[1]);const fs=require('fs');const crypto=require('crypto');"
    "const inp=JSON.parse(fs.readFileSync(process.argv[2],'utf8'));"
    "const out=inp.map(h=>{const u=new Uint8Array(Buffer.from(h,'hex'));"
    "try{const d=Buffer.from(Z.deflate(u));return {len:d.length,sha:crypto.createHash('sha256').update(d).digest('hex')};}"
    "catch(e){return {e:e.message};}});"
    "console.log(JSON.stringify(out));"
)
with tempfile.TemporaryDirectory() as td:
    req = os.path.join(td, "req.json")
    with open(req, "w") as f:
        json.dump([a.tobytes().hex() for a in inputs], f)
    res = json.loads(subprocess.check_output(["node", "-e", js, bundle, req], timeout=600))
out = []
for a, r in zip(inputs, res):
    e = {"n": int(a.size), "input_sha256": hashlib.sha256(a.tobytes()).hexdigest()}
    if "e" in r:
        e["error"] = r["e"]
    else:
        e.update(deflate_len=r["len"], deflate_sha256=r["sha"])
    out.append(e)
with open(os.path.join(HERE, "live_reference.json"), "w") as f:
    json.dump(out, f, indent=0)
    f.write("\n")
print("live_reference.json: %d inputs, %d errors" % (len(out), sum("error" in e for e in out)))
