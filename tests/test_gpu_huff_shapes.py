"""k_huff at the shapes where its teams change: the lit/len team of five wavefronts, the distance wavefront beside it
and the one-wavefront code-length code, against the CPU oracle — code lengths per alphabet, then whole streams."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 131072
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]


# ---------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------
def _fib(k):
    f = [1, 1]
    while len(f) < 24:
        f.append(f[-1] + f[-2])
    return np.array([f[i % 24] for i in range(k)], dtype=np.uint32)  # (sums stay far below 2^32)


def _one_big(k):
    c = np.ones(k, dtype=np.uint32)
    if k:
        c[k // 2] = 131072
    return c


COUNTS = {
    "equal": lambda k: np.full(k, 7, dtype=np.uint32),                                  # every comparison a tie
    "pow2": lambda k: (1 << (np.arange(k) % 17)).astype(np.uint32),                     # package weights equal leaf weights
    "fib": _fib,                                                                         # the limit bites
    "one_big": _one_big,
    "ascending": lambda k: np.arange(1, k + 1, dtype=np.uint32),
    "descending": lambda k: np.arange(k, 0, -1).astype(np.uint32),
}


def length_cases(nsym):
    rng = np.random.default_rng(nsym)
    for k in sorted({0, 1, 2, 3, 63, 64, 65, 255, 256, 257, nsym}):
        if k > nsym:
            continue
        for spread in ("first", "scattered"):
            used = np.arange(k) if spread == "first" else np.sort(rng.choice(nsym, k, replace=False))
            for name, counts in COUNTS.items():
                hist = np.zeros(nsym, dtype=np.uint32)
                hist[used] = counts(k)
                yield "%d used (%s), %s" % (k, spread, name), hist


@pytest.mark.parametrize("nsym,maxlen", [(286, 15), (30, 15), (19, 7)])
def test_lengths_by_used_symbols_and_counts(z, oracle, gpu, nsym, maxlen):
    ran = deepest = 0
    for what, hist in length_cases(nsym):
        got = np.asarray(z.stage_huff_lengths(hist, maxlen))
        want = oracle.huff_lengths(hist, maxlen)
        assert (got == want).all(), "%d symbols, limit %d: %s" % (nsym, maxlen, what)
        ran += 1
        deepest = max(deepest, int(want.max()))
    assert ran == 6 * 2 * (11 if nsym == 286 else 5)
    assert deepest == maxlen  # (the limit was reached: the cases were not all of the easy kind)


# ---------------------------------------------------------------------------------------------
# whole kernel
# ---------------------------------------------------------------------------------------------
def used_symbols(tokens):
    """(used lit/len symbols, the end-of-block code among them; used distance symbols) of a block's token list."""
    tokens = np.asarray(tokens, dtype=np.uint32)
    m = (tokens >> 31) == 1
    lits = np.unique(tokens[~m])
    lens = ((tokens[m] >> 16) & 0x1FF) + 3
    dists = (tokens[m] & 0xFFFF) + 1
    lsym = np.unique(np.searchsorted(_LEN_BASE, lens, side="right"))
    dsym = np.unique(np.searchsorted(_DIST_BASE, dists, side="right"))
    return lits.size + 1 + lsym.size, dsym.size


def planted_block(seed, n=BLOCK):
    """Random bytes with copies planted at distances over 1..32768 and lengths over 3..258: both alphabets large."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    dists = sorted(set(_DIST_BASE) | {32768, 20000, 300, 5})
    p, k = 33000, 0
    while p + 258 + 64 < n:
        d = dists[k % len(dists)]
        ln = 3 + (k * 37) % 256
        for j in range(ln):  # (byte by byte: a copy may overlap its source)
            x[p + j] = x[p + j - d]
        p += ln + 40 + (k % 7)
        k += 1
    return x


@pytest.fixture(scope="module")
def planted():
    return planted_block(11)


def same_stream(z, oracle, x):
    got = np.asarray(z.deflate(x))
    want = oracle.deflate(x)
    assert got.shape == want.shape and (got == want).all()


def test_two_bytes(z, oracle, gpu):
    same_stream(z, oracle, np.array([7, 200], dtype=np.uint8))


def test_no_match_distance_alphabet_empty(z, oracle, gpu):
    x = np.random.default_rng(3).integers(0, 256, 600, dtype=np.uint8)
    assert used_symbols(oracle.lz77_block(x, 0, x.size))[1] == 0
    same_stream(z, oracle, x)


def test_one_distance_symbol(z, oracle, gpu):
    x = np.random.default_rng(3).integers(0, 256, 600, dtype=np.uint8)
    x = np.concatenate([x[:300], x[100:112], x[300:]])
    assert used_symbols(oracle.lz77_block(x, 0, x.size))[1] == 1
    same_stream(z, oracle, x)


def test_both_alphabets_large(z, oracle, gpu, planted):
    nl, nd = used_symbols(oracle.lz77_block(planted, 0, planted.size))
    assert nl > 256 and nd >= 20, (nl, nd)
    same_stream(z, oracle, planted)


def test_batch_of_more_blocks_than_the_machine_holds_at_once(z, oracle, gpu, planted):
    """More than 512 blocks of unlike alphabets in one launch: workgroups of k_huff follow each other on a compute unit."""
    rng = np.random.default_rng(21)
    bufs = [planted]
    for i in range(520):
        n = 2 + (i * 53) % 900
        x = rng.integers(0, 1 + (i % 9) * 31, n, dtype=np.uint8)  # alphabets of 1 .. 249 literals
        if i % 3 == 0 and n > 40:
            x[n // 2:n // 2 + 20] = x[:20]  # a match
        bufs.append(x)
    assert sum((b.size + BLOCK - 1) // BLOCK for b in bufs) > 512
    got = z.deflate_batch(bufs)
    for i, (g, b) in enumerate(zip(got, bufs)):
        want = oracle.deflate(b)
        assert isinstance(g, np.ndarray) and g.shape == want.shape and (g == want).all(), i


def test_two_blocks_first_planted(z, oracle, gpu, planted):
    tail = np.random.default_rng(12).integers(0, 64, 4096, dtype=np.uint8)
    x = np.concatenate([planted, tail])
    assert x.size == BLOCK + 4096
    same_stream(z, oracle, x)
