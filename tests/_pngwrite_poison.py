"""The PNG writer's part of the poison catalogue (tests/_poison_cases.py), registered as tests/_zipwrite_poison.py registers the
ZIP writer's: catalogue entries that call zes_pngwrite_dev and zes_pngwrite on images of tests/_pngwrite.py — a part of the
geometry table as one batch, and nine images that go in groups of four under ZES_F_PIECES — with the files the model and the CPU
oracle give as the expected value, their COVERS lines, and the reason why zes_pngwrite_bound needs none.  Importing this module
adds them to the catalogue (once); tests/test_pngwrite_cpu.py and tests/test_gpu_pngwrite.py import it."""
import _poison_cases as P
import _pngwrite as W

COVERS = {"zes_pngwrite_dev": ["pngwrite_dev *"], "zes_pngwrite": ["host pngwrite *"]}
EXEMPT = {"zes_pngwrite_bound": "host arithmetic only: it touches no device"}


def entries(z, oracle):
    lists = (("part of the geometry table", lambda: W.geometry()[::3], 0), ("nine images in pieces", W.nine, W.PIECES))

    def want(ims):
        b = b"".join(W.expect(im, oracle)[0] for im in ims())
        return ("out", len(b), P.sha(b))

    def run_dev(z, gpu, oracle, ims, flags):
        host, off, out_len, status = W.run_dev(z, gpu, ims(), flags)
        if any(status):
            return ("err", next(s for s in status if s))
        b = b"".join(host[o:o + n].tobytes() for o, n in zip(off, out_len))
        return ("out", len(b), P.sha(b))

    def run_host(z, gpu, oracle, ims, flags):
        res = W.run_host(z, ims(), flags)
        if any(isinstance(r, int) for r in res):
            return ("err", next(r for r in res if isinstance(r, int)))
        b = b"".join(res)
        return ("out", len(b), P.sha(b))

    out = []
    for tag, ims, flags in lists:
        out.append(P.Entry("pngwrite_dev %s" % tag, ["zes_pngwrite_dev"], lambda z, gpu, oracle, ims=ims, flags=flags: run_dev(z, gpu, oracle, ims, flags),
                           lambda ims=ims: want(ims), "oracle"))
        out.append(P.Entry("host pngwrite %s" % tag, ["zes_pngwrite"], lambda z, gpu, oracle, ims=ims, flags=flags: run_host(z, gpu, oracle, ims, flags),
                           lambda ims=ims: want(ims), "oracle"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_pngwrite_registered", False):
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
    P._pngwrite_registered = True


register()
