"""GPU tests of bgzf_inflate_kernel through vb2_bgzf_inflate: no zlib fallback and no CRC32 on this
path, so what comes back is the kernel's.  The streams are the corpus of the CPU check (tests/test_bgzf_inflate_cpu.py),
rebuilt by tests/bgzf_ref.py; the only broken input the kernel is given are the twenty mutilated streams whose statuses
that check decided."""
import os
import sys
import zlib

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgzf_ref as bz  # noqa: E402
from test_bgzf_inflate_cpu import bam_record_bytes  # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    """[(name, BGZF block, plain)] of every corpus stream that fits a BGZF block (a block is at most 65 536 bytes long: the
    incompressible streams of 65 280 bytes and more do not)"""
    out, left = [], 0
    for name, raw, plain in bz.corpus(bam_record_bytes()):
        blk = bz.bgzf_wrap(raw, plain)
        if blk is None:
            left += 1
            continue
        assert zlib.decompress(raw, -15) == plain
        out.append((name, blk, plain))
    assert len(out) > 2400 and left < 250, (len(out), left)
    return out


def _inflate(blocks):
    data, st = vb.api.bgzf_inflate(b"".join(blocks))
    return data, [int(s) for s in st]


@gpu
def test_corpus_inflates_to_zlibs_bytes(corpus):
    data, st = _inflate([b for _, b, _ in corpus])
    assert len(st) == len(corpus)
    bad = [corpus[i][0] for i, s in enumerate(st) if s != 0]
    assert not bad, (len(bad), bad[:10], [s for s in st if s][:10])
    o = 0
    for name, _, plain in corpus:
        assert data[o:o + len(plain)] == plain, name
        o += len(plain)
    assert o == len(data)
    assert {len(p) for _, _, p in corpus} >= {0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65280, 65536}


@pytest.fixture(scope="module")
def mixed(corpus):
    """blocks of every payload length from 0 to 65 280 the corpus has, in an order that mixes them"""
    pick = [c for c in corpus if len(c[2]) <= 65280]
    pick.sort(key=lambda c: zlib.crc32(c[0].encode()))
    assert {0, 65280} <= {len(c[2]) for c in pick[:1025]}
    return pick


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_files_of_n_blocks(mixed, n):
    part = mixed[7:7 + n]
    data, st = _inflate([b for _, b, _ in part])
    assert st == [0] * n
    assert data == b"".join(p for _, _, p in part)


@gpu
def test_a_file_over_three_batches_gives_the_same_bytes(mixed, tunable):
    part = mixed[:1025]
    blocks = [b for _, b, _ in part]
    vb.api.bgzf_inflate_stats(reset=True)
    one, st1 = _inflate(blocks)
    s1 = vb.api.bgzf_inflate_stats(reset=True)
    tunable("bam_batch_kb", 1024)
    many, st2 = _inflate(blocks)
    s2 = vb.api.bgzf_inflate_stats(reset=True)
    print(s1, s2)
    assert s1["batches"] == 1 and s2["batches"] >= 3 and s1["blocks"] == s2["blocks"] == 1025
    assert st1 == st2 == [0] * 1025
    assert many == one == b"".join(p for _, _, p in part)
    assert s2["bytes_inflated"] == len(one) and s2["refused"] == 0


@gpu
def test_broken_streams_give_the_cpu_checks_statuses_and_spare_their_neighbours(mixed):
    small = bz.small_streams()
    good = mixed[40:40 + len(bz.MUTILATED) + 1]
    blocks, want_st, want = [good[0][1]], [0], [good[0][2]]
    for (name, kind, index, status), g in zip(bz.MUTILATED, good[1:]):
        raw, plain = small[name]
        blocks.append(bz.bgzf_wrap(bz.mutilate(raw, kind, index), plain))          # (ISIZE and CRC32 of the unbroken stream)
        want_st.append(status)
        want.append(bytes(len(plain)))                                            # a refused block's bytes are zero
        blocks.append(g[1])
        want_st.append(0)
        want.append(g[2])
    data, st = _inflate(blocks)
    assert st == want_st
    assert data == b"".join(want)


@gpu
def test_a_buffer_that_is_not_bgzf_is_refused_with_the_readers_message(mixed):
    from verifybamid_amd import _abi
    blk = mixed[3][1]
    for broken, word in ((blk[:10], "truncated header"), (b"\x1f\x8c" + blk[2:], "bad magic"), (blk + blk[:30], "passes the end")):
        with pytest.raises(_abi.Vb2Error):
            vb.api.bgzf_inflate(broken)
        assert word in _abi.lib().vb2_last_error().decode()
    assert vb.api.bgzf_inflate(b"")[0] == b""
