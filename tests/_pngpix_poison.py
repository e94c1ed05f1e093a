"""The PNG pixel forms' part of the poison catalogue (tests/_poison_cases.py), registered as tests/_png_poison.py registers the
reader's: catalogue entries that call zes_pngpix_dev, zes_pngpix_alloc and zes_pngpix_expand_dev on the images of
tests/_pngpix.py — a part of the case table that spans the pairs and the kinds, and the reader's damage table between good
neighbours (for the expand call: records the writer's rule refuses between good ones) — and their COVERS lines.  Importing
this module adds them to the catalogue (once); tests/test_pngpix_cpu.py and tests/test_gpu_pngpix.py import it.

Streams are CPython's zlib's and the expected pixels are the numpy rule's over the writer's inputs, so no entry's value comes
from the library."""
import functools

import numpy as np

import _pngpix as X
import _poison_cases as P

COVERS = {"zes_pngpix_dev": ["pngpix_dev *"], "zes_pngpix_alloc": ["host pngpix *"], "zes_pngpix_expand_dev": ["pngpix_expand_dev *"]}
EXEMPT = {}
ZES_E_ARG = -18


def entries(z, oracle):
    good = functools.lru_cache(maxsize=None)(lambda: [(c.blob, 0, c.want) for c in X.subset()])
    damaged = functools.lru_cache(maxsize=None)(lambda: [(blob, st, want) for _, blob, st, want in X.damaged()])
    either = lambda want: ("err", "one of %r" % (want,))  # the stream cut short: the inflate tiers' status, or -21

    def want(rows):
        return [("out", w.size, P.sha(w)) if st == 0 else either(st) if isinstance(st, tuple) else ("err", st) for _, st, w in rows]

    def told(rows, status, datas):
        return [("out", len(d), P.sha(d)) if s == 0 else either(st) if isinstance(st, tuple) and s in st else ("err", s)
                for (_, st, _), s, d in zip(rows, status, datas)]

    def run_dev(z, gpu, oracle, rows):
        flat, off, ln = X.pack([r[0] for r in rows()])
        out, ooff, out_len, status, _ = z.png_pixels_tensor(P.dev(flat, gpu), off, ln)
        host = out.cpu().numpy()
        return told(rows(), status, [host[int(o):int(o) + n].tobytes() if s == 0 else b"" for o, n, s in zip(ooff, out_len, status)])

    def run_host(z, gpu, oracle, rows):
        res = z.png_pixels_batch([r[0] for r in rows()])
        return told(rows(), [r.code if isinstance(r, Exception) else 0 for r in res], [b"" if isinstance(r, Exception) else r[1].tobytes() for r in res])

    # the expand call: the scanlines themselves; `refused`: every third record gets a depth its colour type does not have
    fitting = functools.lru_cache(maxsize=None)(lambda: [c for c in X.subset() if c.fits])

    def records(refused):
        img = np.zeros(len(fitting()), dtype=[("width", "<u4"), ("height", "<u4"), ("depth", "u1"), ("colour", "u1"), ("filter", "u1"), ("pad", "u1"),
                                              ("plte_len", "<u2"), ("trns_len", "<u2")])
        for i, c in enumerate(fitting()):
            img[i] = c.record()
            if refused and i % 3 == 1:
                img[i]["depth"] = 3
        return img

    def want_expand(refused):
        return [("err", ZES_E_ARG) if refused and i % 3 == 1 else ("out", c.want.size, P.sha(c.want)) for i, c in enumerate(fitting())]

    def run_expand(z, gpu, oracle, refused):
        cs = fitting()
        flat, off, ln = X.pack([c.raw for c in cs])
        out, ooff, out_len, status = z.png_expand_tensor(P.dev(flat, gpu), off, ln, records(refused), b"".join(c.plte + c.trns for c in cs))
        host = out.cpu().numpy()
        return [("out", n, P.sha(host[int(o):int(o) + n])) if s == 0 else ("err", s) for o, n, s in zip(ooff, out_len, status)]

    out = []
    for tag, rows in (("good images", good), ("damaged images", damaged)):
        out.append(P.Entry("pngpix_dev %s" % tag, ["zes_pngpix_dev"], lambda z, gpu, oracle, rows=rows: run_dev(z, gpu, oracle, rows),
                           lambda rows=rows: want(rows()), "zlib"))
        out.append(P.Entry("host pngpix %s" % tag, ["zes_pngpix_alloc"], lambda z, gpu, oracle, rows=rows: run_host(z, gpu, oracle, rows),
                           lambda rows=rows: want(rows()), "zlib"))
    for tag, refused in (("good images", False), ("refused records between good ones", True)):
        out.append(P.Entry("pngpix_expand_dev %s" % tag, ["zes_pngpix_expand_dev"], lambda z, gpu, oracle, refused=refused: run_expand(z, gpu, oracle, refused),
                           lambda refused=refused: want_expand(refused), "zlib"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS lines beside its own; a second call does nothing."""
    if getattr(P, "_pngpix_registered", False):
        return
    P._CATALOGUE.clear()  # (built already: it is built again, with these entries, at its next use)
    base = P.build

    def build(z, oracle):
        got = base(z, oracle) + entries(z, oracle)
        names = [e.name for e in got]
        assert len(set(names)) == len(names)
        return got

    P.build = build
    P.COVERS.update(COVERS)
    P.EXEMPT.update(EXEMPT)
    P._pngpix_registered = True


register()
