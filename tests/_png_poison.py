"""The PNG reader's part of the poison catalogue (tests/_poison_cases.py), registered as tests/_zip_poison.py registers the ZIP
reader's: four catalogue entries that call zes_png_decode_dev / zes_png_decode_alloc on files of tests/_png.py (a part of the
geometry table; the damage table between good neighbours), their COVERS lines, and the reason why the info call needs none.
Importing this module adds them to the catalogue (once): tests/test_png_cpu.py and tests/test_gpu_png.py import it.

Streams are CPython's zlib's and the expected bytes are the writer's inputs, so no entry's value comes from the library."""
import functools

import numpy as np

import _png
import _poison_cases as P

COVERS = {"zes_png_decode_dev": ["png_decode_dev *"], "zes_png_decode_alloc": ["host png_decode *"]}
EXEMPT = {"zes_png_info_get": "the host form walks the caller's memory on the host and touches no device"}


def entries(z, oracle):
    good = functools.lru_cache(maxsize=None)(lambda: [(c.blob, 0, c.want) for c in _png.geometry()[::4]])

    @functools.lru_cache(maxsize=None)
    def damaged():
        a, b = _png.neighbours()
        rows = [(a.blob, 0, a.want)]
        for c in _png.damage():
            if not c.short:
                rows += [(c.blob, c.status, c.want), (b.blob, 0, b.want)]
        return rows

    either = lambda want: ("err", "one of %r" % (want,))  # the stream cut short: the inflate tiers' status, or -21

    def want(rows):
        return [("out", len(data), P.sha(data)) if w == 0 else either(w) if isinstance(w, tuple) else ("err", w) for _, w, data in rows]

    def told(rows, status, datas):
        return [("out", len(d), P.sha(d)) if s == 0 else either(w) if isinstance(w, tuple) and s in w else ("err", s)
                for (_, w, _), s, d in zip(rows, status, datas)]

    def run_dev(z, gpu, oracle, rows):
        blobs = [r[0] for r in rows()]
        off = np.cumsum([1] + [len(b) + 3 for b in blobs])[:-1]  # files at any byte
        flat = np.zeros(int(off[-1]) + len(blobs[-1]), dtype=np.uint8)
        for o, b in zip(off, blobs):
            flat[int(o):int(o) + len(b)] = P.u8(b)
        out, ooff, out_len, status, _ = z.png_decode_tensor(P.dev(flat, gpu), off, [len(b) for b in blobs])
        host = out.cpu().numpy()
        return told(rows(), status, [host[int(o):int(o) + n].tobytes() for o, n in zip(ooff, out_len)])

    def run_host(z, gpu, oracle, rows):
        res = z.png_decode_batch([r[0] for r in rows()])
        return told(rows(), [r.code if isinstance(r, Exception) else 0 for r in res], [b"" if isinstance(r, Exception) else r[1].tobytes() for r in res])

    out = []
    for tag, rows in (("good images", good), ("damaged images", damaged)):
        out.append(P.Entry("png_decode_dev %s" % tag, ["zes_png_decode_dev"], lambda z, gpu, oracle, rows=rows: run_dev(z, gpu, oracle, rows),
                           lambda rows=rows: want(rows()), "zlib"))
        out.append(P.Entry("host png_decode %s" % tag, ["zes_png_decode_alloc"], lambda z, gpu, oracle, rows=rows: run_host(z, gpu, oracle, rows),
                           lambda rows=rows: want(rows()), "zlib"))
    return out


def register():
    """The entries behind the catalogue's own, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_png_registered", False):
        return
    P._CATALOGUE.clear()  # (built already: it is built again, with the PNG entries, at its next use)
    base = P.build

    def build(z, oracle):
        got = base(z, oracle) + entries(z, oracle)
        names = [e.name for e in got]
        assert len(set(names)) == len(names)
        return got

    P.build = build
    P.COVERS.update(COVERS)
    P.EXEMPT.update(EXEMPT)
    P._png_registered = True


register()
