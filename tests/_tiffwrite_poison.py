"""The TIFF writer's part of the poison catalogue (tests/_poison_cases.py), registered as tests/_tiff_poison.py registers the
reader's: catalogue entries that write images of tests/_tiffwrite.py's tables through the device form (zes_tiffwrite_dev) and the
host form (zes_tiffwrite), with the file its restated layout and the CPU oracle give as the expected value; their COVERS lines,
and the reason why zes_tiffwrite_bound needs none.  Importing this module adds them to the catalogue (once);
tests/test_tiffwrite_cpu.py and tests/test_gpu_tiffwrite.py import it."""
import _poison_cases as P
import _tiffwrite as W

COVERS = {"zes_tiffwrite_dev": ["tiffwrite_dev *"], "zes_tiffwrite": ["host tiffwrite *"]}
EXEMPT = {"zes_tiffwrite_bound": "host arithmetic only: it touches no device"}

# tiles with zero columns and rows under Predictor 2 (what the cut kernel leaves unwritten would show), strips in two groups
# under ZES_F_PIECES, and both routes in one image
CASES = (("six tiles", W.six_tiles, 0), ("six tiles in pieces", W.six_tiles, W.PIECES), ("mixed routes", W.mixed, 0),
         ("strips, 16 bits x 3, MM", lambda: next(c for c in W.grid(layouts=(("strips", 5),), depths=(16,), samples=(3,), orders=("MM",), codings=((8, 2),))), W.PIECES))


def entries(z, oracle):
    def want(case):
        b = W.expect(case(), oracle)[0]
        return ("out", len(b), P.sha(b))

    def run_dev(z, gpu, oracle, case, flags):
        b, _, _ = W.run_dev(z, gpu, case(), at=1, flags=flags)
        return ("out", len(b), P.sha(b))

    def run_host(z, gpu, oracle, case, flags):
        b = W.run_host(z, case(), flags)
        return ("out", len(b), P.sha(b))

    out = []
    for tag, case, flags in CASES:
        out.append(P.Entry("tiffwrite_dev %s" % tag, ["zes_tiffwrite_dev"], lambda z, gpu, oracle, case=case, flags=flags: run_dev(z, gpu, oracle, case, flags),
                           lambda case=case: want(case), "oracle"))
        out.append(P.Entry("host tiffwrite %s" % tag, ["zes_tiffwrite"], lambda z, gpu, oracle, case=case, flags=flags: run_host(z, gpu, oracle, case, flags),
                           lambda case=case: want(case), "oracle"))
    return out


def register():
    """The entries behind the catalogue's, the COVERS and EXEMPT lines beside its own; a second call does nothing."""
    if getattr(P, "_tiffwrite_registered", False):
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
    P._tiffwrite_registered = True


register()
