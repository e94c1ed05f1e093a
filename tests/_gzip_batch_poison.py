"""The gzip batch forms' part of the poison catalogue (tests/_poison_cases.py), registered as tests/_zipwrite_poison.py registers
the ZIP writer's: catalogue entries that call zes_gzip_batch_dev and zes_gzip_batch on the writer's case list of
tests/_gzip_batch.py (the host form on the nine buffers that go in groups of four under ZES_F_PIECES), with the files its builder
and the CPU oracle give as the expected value, and entries that call zes_gunzip_batch_dev and zes_gunzip_batch_alloc on the
reader's files of both routes, with CPython's bytes and the statuses of include/zes.h as the expected value; their COVERS lines,
and the reason why zes_gzip_batch_bound needs none.  Importing this module adds them to the catalogue (once);
tests/test_gzip_batch_cpu.py and tests/test_gpu_gzip_batch.py import it."""
import numpy as np

import _gzip_batch as G
import _poison_cases as P

COVERS = {"zes_gzip_batch_dev": ["gzip_batch_dev *"], "zes_gzip_batch": ["host gzip_batch *"], "zes_gunzip_batch_dev": ["gunzip_batch_dev *"],
          "zes_gunzip_batch_alloc": ["host gunzip_batch *"], "zes_last_gunzip_batch": ["gunzip_batch_dev *", "host gunzip_batch *"]}
EXEMPT = {"zes_gzip_batch_bound": "host arithmetic only: it touches no device"}

# the files of the per-file route whose status include/zes.h states outright (zes_gunzip*)
STATED = {"two members": G.OK, "a BGZF file of 3 members and the marker": G.OK, "trailing zero bytes": G.OK, "FHCRC right": G.OK,
          "FHCRC wrong": G.E_CHECKSUM, "an FNAME of 300 bytes": G.OK, "bad magic": G.E_GZIP, "CM 9": G.E_GZIP, "a reserved FLG bit": G.E_GZIP,
          "no bytes": G.E_GZIP, "a wrong CRC": G.E_CHECKSUM, "ISIZE one less": G.E_CHECKSUM, "40 bytes claiming 0xFFFFFFF0": G.E_CHECKSUM}


def reader_files(z):
    """[(file, expected)]: the good files and the stated ones of the per-file route, interleaved; expected is ("out", n, sha) or
    ("err", status)."""
    good = [(f, ("out", len(p), P.sha(p))) for _, f, p in G.good_files(z)]
    bad = [(f, ("out", len(v), P.sha(v)) if STATED[n] == G.OK else ("err", STATED[n])) for n, f, v, _ in G.serial_files(z) if n in STATED]
    out = []
    for k in range(max(len(good), len(bad))):
        out += good[k:k + 1] + bad[k:k + 1]
    return out


def _layout(blobs, lead=3):
    blob = b"".join(blobs)
    off = np.cumsum([lead] + [len(b) for b in blobs])[:-1]
    return np.concatenate([np.zeros(lead, dtype=np.uint8), P.u8(blob)]), off, [len(b) for b in blobs]


def _value(items):
    return tuple(("err", x.code) if isinstance(x, Exception) else ("out", int(len(x)), P.sha(x)) for x in items)


def entries(z, oracle):
    def want_files(es):
        return tuple(("out", len(f), P.sha(f)) for f in (G.expect(d)[0] for _, d in es()))

    def gzip_dev(z, gpu, oracle, es, flags):
        t, off, ln = _layout([d for _, d in es()])
        out, o, n, st = z.gzip_batch_tensor(P.dev(t, gpu), off, ln, flags=flags)
        host = out.cpu().numpy()
        return tuple(("out", n[i], P.sha(host[int(o[i]):int(o[i]) + n[i]])) if st[i] == 0 else ("err", st[i]) for i in range(len(ln)))

    def gunzip_dev(z, gpu, oracle, flags):
        fs = reader_files(z)
        t, off, ln = _layout([f for f, _ in fs])
        sizes = [w[1] if w[0] == "out" else 0 for _, w in fs]
        at = np.cumsum([5] + [s + 3 for s in sizes])  # the outputs at odd bytes, three bytes between them
        import torch

        out = torch.zeros(int(at[-1]), dtype=torch.uint8, device=gpu)
        _, _, n, st = z.gunzip_batch_tensor(P.dev(t, gpu), off, ln, out=out, off=at[:-1], cap=sizes, flags=flags)
        host = out.cpu().numpy()
        got = tuple(("out", n[i], P.sha(host[int(at[i]):int(at[i]) + n[i]])) if st[i] == 0 else ("err", st[i]) for i in range(len(ln)))
        return got, z.last_gunzip_batch()

    def gunzip_host(z, gpu, oracle, flags):
        return _value(z.gunzip_batch([f for f, _ in reader_files(z)], flags)), z.last_gunzip_batch()

    def want_reader():
        fs = reader_files(z)
        nbad = sum(1 for n in [x[0] for x in G.serial_files(z)] if n in STATED)
        return tuple(w for _, w in fs), (len(fs) - nbad, nbad)

    lists = (("case list", lambda: G.writer_cases(z), 0), ("nine buffers in pieces", lambda: G.nine(z), G.PIECES))
    out = []
    for tag, es, flags in lists:
        out.append(P.Entry("gzip_batch_dev %s" % tag, ["zes_gzip_batch_dev"], lambda z, gpu, oracle, es=es, flags=flags: gzip_dev(z, gpu, oracle, es, flags),
                           lambda es=es: want_files(es), "oracle"))
        out.append(P.Entry("host gzip_batch %s" % tag, ["zes_gzip_batch"],
                           lambda z, gpu, oracle, es=es, flags=flags: _value(z.gzip_batch([d for _, d in es()], flags)), lambda es=es: want_files(es), "oracle"))
    out.append(P.Entry("gunzip_batch_dev both routes", ["zes_gunzip_batch_dev", "zes_last_gunzip_batch"], lambda z, gpu, oracle: gunzip_dev(z, gpu, oracle, 0),
                       want_reader, "zlib"))
    out.append(P.Entry("host gunzip_batch both routes", ["zes_gunzip_batch_alloc", "zes_last_gunzip_batch"], lambda z, gpu, oracle: gunzip_host(z, gpu, oracle, 0),
                       want_reader, "zlib"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_gzip_batch_registered", False):
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
    P._gzip_batch_registered = True


register()
