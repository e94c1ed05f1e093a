"""The ZIP writer's part of the poison catalogue (tests/_poison_cases.py), registered as tests/_zip_poison.py registers the
reader's: catalogue entries that call zes_zipwrite_dev and zes_zipwrite on the case list of tests/_zipwrite.py — as one archive,
as the nine entries that go in groups of four under ZES_F_PIECES and as six whose groups end at the bytes of their slots — with the archive the builder and the CPU oracle give as the
expected value, their COVERS lines, and the reason why zes_zipwrite_bound needs none.  Importing this module adds them to the
catalogue (once); tests/test_zipwrite_cpu.py and tests/test_gpu_zipwrite.py import it."""
import numpy as np

import _poison_cases as P
import _zipwrite as W

COVERS = {"zes_zipwrite_dev": ["zipwrite_dev *"], "zes_zipwrite": ["host zipwrite *"]}
EXEMPT = {"zes_zipwrite_bound": "host arithmetic only: it touches no device"}


def entries(z, oracle):
    lists = (("case list", lambda: W.cases(z), 0), ("nine entries in pieces", lambda: W.nine(z), W.PIECES),
             ("six entries in groups that end at their slots", lambda: W.slots(z), W.PIECES))

    def want(es):
        b = W.expect(es())
        return ("out", len(b), P.sha(b))

    def run_dev(z, gpu, oracle, es, flags):
        es = es()
        blob = b"".join(d for _, d in es)
        off = np.cumsum([0] + [len(d) for _, d in es])[:-1]
        t = P.dev(np.concatenate([np.zeros(3, dtype=np.uint8), P.u8(blob)]), gpu)[3:]
        return P.outcome(z, lambda: z.zip_write_tensor(t, off, [len(d) for _, d in es], [n for n, _ in es], flags=flags)[0])

    def run_host(z, gpu, oracle, es, flags):
        return P.outcome(z, lambda: z.zip_write(es(), flags=flags)[0])

    out = []
    for tag, es, flags in lists:
        out.append(P.Entry("zipwrite_dev %s" % tag, ["zes_zipwrite_dev"], lambda z, gpu, oracle, es=es, flags=flags: run_dev(z, gpu, oracle, es, flags),
                           lambda es=es: want(es), "oracle"))
        out.append(P.Entry("host zipwrite %s" % tag, ["zes_zipwrite"], lambda z, gpu, oracle, es=es, flags=flags: run_host(z, gpu, oracle, es, flags),
                           lambda es=es: want(es), "oracle"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_zipwrite_registered", False):
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
    P._zipwrite_registered = True


register()
