"""The TIFF reader's part of the poison catalogue (tests/_poison_cases.py), registered as tests/_gzip_batch_poison.py registers
the gzip batch forms': catalogue entries that index and read files of tests/_tiff.py's case table through the device form
(zes_tiff_index_dev, zes_tiff_read_dev) and the host form (zes_tiff_read_alloc), with the pixels its independent reader gives
as the expected value; their COVERS lines, and the reason why zes_tiff_index needs none.  Importing this module adds them to
the catalogue (once); tests/test_tiff_cpu.py and tests/test_gpu_tiff.py import it."""
import numpy as np

import _poison_cases as P
import _tiff as T

COVERS = {"zes_tiff_index_dev": ["tiff_read_dev *"], "zes_tiff_read_dev": ["tiff_read_dev *"], "zes_tiff_read_alloc": ["host tiff_read *"],
          "zes_last_tiff_read": ["tiff_read_dev *", "host tiff_read *"]}
EXEMPT = {"zes_tiff_index": "the host form applies the file rule to the caller's memory on the host and touches no device"}

FILES = (
    ("tiles, 16 bits x 3, MM, Predictor 2", dict(w=37, h=23, spp=3, bits=16, layout=("tiles", 16, 16), order="MM", compression=8, predictor=2), (27, 9, 8, 11)),
    ("strips of 5, 8 bits x 4, Predictor 2", dict(w=37, h=23, spp=4, bits=8, layout=("strips", 5), order="II", compression=32946, predictor=2), None),
    ("tiles, 32 bits, uncompressed", dict(w=37, h=23, spp=1, bits=32, layout=("tiles", 32, 16), order="MM", compression=1, predictor=1), (3, 2, 30, 20)),
)


def _want(kw, rect):
    f, _ = T.make(**kw)
    rec = T.rule(f)[0]
    px = T.decode(f, 0, rect)
    return ("out", int(px.nbytes), P.sha(px.view(np.uint8))), len(T.touched(rec, rect or (0, 0, rec["width"], rec["height"])))


def entries(z, oracle):
    def run_dev(z, gpu, oracle, kw, rect):
        f, _ = T.make(**kw)
        t = P.dev(np.concatenate([np.zeros(1, dtype=np.uint8), P.u8(f)]), gpu)[1:]
        out, st, rc = z.tiff_read_tensor(t, z.tiff_index_tensor(t), rect)
        assert rc == 0 and not st.any()
        host = out.cpu().numpy()
        return ("out", int(host.size), P.sha(host)), z.last_tiff_read()[0]

    def run_host(z, gpu, oracle, kw, rect):
        f, _ = T.make(**kw)
        px = z.tiff_read(f, 0, rect)
        return ("out", int(px.nbytes), P.sha(px.view(np.uint8))), z.last_tiff_read()[0]

    out = []
    for name, kw, rect in FILES:
        out.append(P.Entry("tiff_read_dev %s" % name, ["zes_tiff_index_dev", "zes_tiff_read_dev", "zes_last_tiff_read"],
                           lambda z, gpu, oracle, kw=kw, rect=rect: run_dev(z, gpu, oracle, kw, rect), lambda kw=kw, rect=rect: _want(kw, rect), "zlib"))
        out.append(P.Entry("host tiff_read %s" % name, ["zes_tiff_read_alloc", "zes_last_tiff_read"],
                           lambda z, gpu, oracle, kw=kw, rect=rect: run_host(z, gpu, oracle, kw, rect), lambda kw=kw, rect=rect: _want(kw, rect), "zlib"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_tiff_registered", False):
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
    P._tiff_registered = True


register()
