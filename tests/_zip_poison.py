"""The ZIP reader's part of the poison catalogue (tests/_poison_cases.py), kept beside the ZIP tests: four catalogue entries that
call zes_zip_read_dev / zes_zip_read_alloc on the archives of tests/_zip.py, their COVERS lines, and the reasons why the two
index forms need none.  Importing this module adds them to the catalogue (once): tests/test_zip_cpu.py and tests/test_gpu_zip.py import it, so wherever
they are collected together with tests/test_poison_cpu.py and tests/test_gpu_poison.py — a run of the suite — those two see
every ZIP entry point covered or exempt and run the ZIP entries under every poison word.  tests/test_zip_cpu.py checks the same
facts for the ZIP entry points alone, whatever else is collected.

Bodies are CPython's zlib's and the index is the restated rule of tests/_zip.py, so that no entry calls zes_zip_index."""
import functools

import numpy as np

import _poison_cases as P
import _zip

COVERS = {"zes_zip_read_dev": ["zip_read_dev *"], "zes_zip_read_alloc": ["host zip_read *"]}
EXEMPT = {
    "zes_zip_index": "the host form walks the caller's memory on the host and touches no device",
    "zes_zip_index_dev": "two copies to host memory and the host form's walk: no kernel, no pool",
}


def entries(z, oracle):
    def index(blob):
        st, ent, _ = _zip.index_rule(blob)
        assert st == 0
        a = np.zeros(len(ent), dtype=z.ZIP_ENTRY)
        for k, e in enumerate(ent):
            for f, v in e.items():
                a[k][f] = v
        return a

    standard = functools.lru_cache(maxsize=None)(lambda: (lambda b, plain, _: (b, [(0, p) for p in plain]))(*_zip.standard()))
    failure = functools.lru_cache(maxsize=None)(lambda: (lambda b, plan: (b, [(want, data) for _, want, data in plan]))(*_zip.failures()))
    either = lambda want: ("err", "one of %r" % (want,))  # the entry whose body is cut short: the inflate tiers' status, or -21

    def want(rows):
        return [("out", len(data), P.sha(data)) if w == 0 else either(w) if isinstance(w, tuple) else ("err", w) for w, data in rows]

    def told(rows, status, datas):
        return [("out", len(d), P.sha(d)) if s == 0 else either(w) if isinstance(w, tuple) and s in w else ("err", s)
                for (w, _), s, d in zip(rows, status, datas)]

    def run_dev(z, gpu, oracle, arch):
        blob, rows = arch()
        out, off, out_len, status = z.zip_read_tensor(P.dev(np.concatenate([np.zeros(1, dtype=np.uint8), P.u8(blob)]), gpu)[1:], index(blob))
        host = out.cpu().numpy()
        return told(rows, status, [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)])

    def run_host(z, gpu, oracle, arch):
        blob, rows = arch()
        res = z.zip_read(blob, index(blob))
        return told(rows, [r.code if isinstance(r, Exception) else 0 for r in res], [b"" if isinstance(r, Exception) else r.tobytes() for r in res])

    out = []
    for tag, arch in (("standard", standard), ("failure", failure)):
        out.append(P.Entry("zip_read_dev %s archive" % tag, ["zes_zip_read_dev"], lambda z, gpu, oracle, arch=arch: run_dev(z, gpu, oracle, arch),
                           lambda arch=arch: want(arch()[1]), "zlib"))
        out.append(P.Entry("host zip_read %s archive" % tag, ["zes_zip_read_alloc"], lambda z, gpu, oracle, arch=arch: run_host(z, gpu, oracle, arch),
                           lambda arch=arch: want(arch()[1]), "zlib"))
    return out


def register():
    """The entries behind the catalogue's own, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_zip_registered", False):
        return
    P._CATALOGUE.clear()  # (built already: it is built again, with the ZIP entries, at its next use)
    base = P.build

    def build(z, oracle):
        got = base(z, oracle) + entries(z, oracle)
        names = [e.name for e in got]
        assert len(set(names)) == len(names)
        return got

    P.build = build
    P.COVERS.update(COVERS)
    P.EXEMPT.update(EXEMPT)
    P._zip_registered = True


register()
