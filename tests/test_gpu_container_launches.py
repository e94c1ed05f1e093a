"""Which launches the checksum / gzip / BGZF / ZIP / PNG layer makes, pinned: every case of tests/_container_cases.py — status, result,
the launch count of each of the layer's kernels and the names of the inflate and deflate kernels beside them — against
tests/golden/container_launches.json, which was recorded from the commits in front of the layer's two refactors (NOTES.md
says which).  A driver that launched a gather twice, walked a file on the device that the host had walked already, or ran a
checksum kernel over buffers of no bytes computes the same values; here it shows as a count.

Every case runs twice in a row on the same context and the second record must equal the first: the pools a call has grown
and the cached CRC table do not reach the next call's launches.
"""
import json

import pytest

import _container_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(K.GOLDEN) as f:
        return json.load(f)


def test_golden_file_has_every_case(golden):
    assert sorted(golden) == sorted(K.CASES)


def facts(name, rec):
    """What a case's record must say whatever was recorded: the values (CPython's zlib, the inputs' own bytes), the statuses
    the streams were built for, and the launches the entry points' descriptions state."""
    n = rec["launches"]
    if name.endswith("damaged"):  # one bit of the 70000-byte BGZF file flipped: the call fails
        assert rec["status"] != 0 and rec["members"] == 0 and rec["out_len"] is None, rec
        if name.startswith("gunzip_tensor"):  # the batch gives up, the serial path answers
            assert rec["status"] == -21 and n.get("k_crc32", 0) >= 1 and "k_crc32_seg" not in n, rec
        elif name.endswith("body damaged"):  # the job's verdict comes before the output gather and the CRC launch
            assert "k_crc32_seg" not in n and "k_crc32" not in n, rec
        else:  # ZES_E_CHECKSUM behind the CRC launch
            assert rec["status"] == -21 and n.get("k_crc32_seg") == 1, rec
        return
    assert rec["status"] == 0, rec
    if name.split()[0] in ("png_decode_tensor", "png_decode"):
        # good, flipped Adler-32, good: one launch of each step for the batch, the walk only where the files are on the device
        assert rec["statuses"] == [0, -21, 0] and rec["bytes_equal"] == [True, None, True] and rec["out_len"][1] == 0, rec
        assert n.get("k_png_walk") == (1 if name.startswith("png_decode_tensor") else None), rec
        assert n.get("k_crc32_seg") == 1 and n.get("k_adler_seg") == 1 and n.get("k_png_unfilter") == 1 and n.get("k_gz_gather", 0) >= 1 and rec["others"], rec
        return
    if name.split()[0] in ("zip_read_tensor", "zip_read"):
        # every status is the one tests/_zip.py expects of the entry (entry_rule), the bytes are the entries' own
        assert all(rec["expected"]) and all(b for b, s in zip(rec["bytes_equal"], rec["statuses"]) if s == 0), rec
        assert all((b is None) == (s != 0) for b, s in zip(rec["bytes_equal"], rec["statuses"])), rec
        if name.endswith("count 0"):
            assert n == {} and not rec["others"] and rec["statuses"] == [], rec  # no launch at all
        elif name.endswith("one rejected"):  # no job at ZES_OK: no decoder, and nothing to gather or to check
            assert rec["statuses"] == [-22] and n == {"k_zip_stage": 1} and not rec["others"], rec
        elif name.endswith("stored only"):  # no job: the copy is the stage kernel's
            assert set(rec["statuses"]) == {0} and n == {"k_zip_stage": 1, "k_crc32_seg": 1} and not rec["others"], rec
        else:  # one stage launch, one CRC launch that covers the good entries beside the damaged ones
            assert n.get("k_zip_stage") == 1 and n.get("k_crc32_seg") == 1 and n.get("k_gz_gather", 0) >= 1 and rec["others"], rec
            good = rec["statuses"].count(0)
            assert good == 18 == len(rec["statuses"]) if name.endswith("standard") else 6 <= good < len(rec["statuses"]), rec
        return
    if name.startswith("zipwrite"):
        groups = 3 if name.endswith("pieces") else 1
        assert rec["sha256_expected"] and n.get("k_crc32_seg") == groups and n.get("k_zip_pack") == groups, rec
        if name.endswith("refused only"):  # no encoder slot: no deflate kernel
            assert set(n) == {"k_crc32_seg", "k_zip_pack"} and not rec["others"] and set(rec["methods"]) == {0}, rec
        else:
            assert rec["others"] and 8 in rec["methods"], rec
        return
    if name == "bgzip_tensor 1 byte":  # the only chunk is one the encoder refuses: a stored member and the marker
        assert rec["bytes_equal"] and rec["out_len"] == 32 + 28 and n == {"k_crc32_seg": 1, "k_bgzf_pack": 1} and not rec["others"], rec
        return
    if "values_equal" in rec:
        assert rec["values_equal"], rec
    if "bytes_equal" in rec and not isinstance(rec["bytes_equal"], list):
        assert rec["bytes_equal"], rec
    if name in ("crc32 batch", "adler32 batch"):
        assert n == {"k_crc32_seg" if name.startswith("crc32") else "k_adler_seg": 1} and not rec["others"], rec
    elif name.endswith("every length 0") or name.endswith("count 0"):
        assert n == {} and not rec["others"], rec  # nothing to do: no launch
    elif name in ("gunzip_tensor bgzf", "gunzip bgzf"):
        assert rec["members"] >= 2 and n.get("k_crc32_seg") == 1 and "k_crc32" not in n, rec
        assert n.get("k_gz_walk") == (1 if name.startswith("gunzip_tensor") else None), rec  # the host form walks the caller's memory
    elif name == "gunzip two members":  # the serial path (a member's inflate call collects the times: the last member's k_crc32 shows)
        assert rec["members"] == 0 and n.get("k_crc32", 0) >= 1 and "k_gz_walk" not in n and "k_crc32_seg" not in n, rec
    elif name in ("bgzip_tensor", "bgzip_tensor pieces"):
        groups = 2 if name.endswith("pieces") else 1
        assert n.get("k_crc32_seg") == groups and n.get("k_bgzf_pack") == groups, rec
    elif name.startswith("bgzf_index_tensor"):
        assert rec["same_as_host_index"], rec
        assert (n.get("k_gz_walk"), n.get("k_bgzf_mark")) == ((1, None) if name.endswith("walk") else (None, 1)), rec
    elif name in ("bgzf_read_tensor", "bgzf_read"):
        assert rec["members"] == 2 and n.get("k_crc32_seg") == 1 and n.get("k_gz_gather", 0) >= 2, rec
    else:  # the checked batches: good, wrong trailer, cut inside the trailer
        assert rec["statuses"] == [0, -21, -21] and rec["bytes_equal"][0] and n.get("k_adler_seg") == 1, rec


@pytest.mark.parametrize("name", K.CASES)
def test_launches(z, gpu, golden, name):
    first = K.run_case(z, gpu, name)
    second = K.run_case(z, gpu, name)
    print(name, first)
    facts(name, first)
    assert first == golden[name], (name, first, golden[name])
    assert second == first, (name, "second run", second, first)
