"""GPU: k_inflate_bgzf on DEFLATE streams that zlib's encoder never writes (tests/deflate_craft.py; the same members go
through the kernel's core on the host in test_deflate_craft_cpu.py, which also asserts what each family holds).  zlib
is the reference: every member's text was decoded by zlib when the member was built."""
import random

import pytest

import deflate_craft as DC
import inflate_cases as IC
from conftest import pkg
from test_device_inflate_gpu import GUIDES, KWS, check_same

pytestmark = pytest.mark.gpu

PADS = [None, 0, 1, 2, 3]


def device_text(members, pad=None):
    with pkg().Counter(features=GUIDES) as c:
        dt, trunc = c.text_from_bgzf(IC.bgzf_wrap(members, pad))
        text = dt.read()
        dt.free()
    return text, trunc


def test_text_from_bgzf_good_members():
    """every good member, then all of them shuffled again and again: over 1100 members on at most 512 workgroups, so each
    workgroup decodes several unlike members in a row on one block of LDS (fixed after dynamic, short tables after long)"""
    rng = random.Random(7)
    once = [(name, m, t) for name, (m, t) in DC.good_members().items()]
    ms = list(once)
    while len(ms) < 1100:
        again = list(once)
        rng.shuffle(again)
        ms += again
    assert len(ms) >= 1100 and len(once) > 200
    text, trunc = device_text([m for _, m, _ in ms], pad=[PADS[i % 5] for i in range(len(ms))])
    assert not trunc and len(text) == sum(len(t) for _, _, t in ms)
    o = 0
    for i, (name, _, t) in enumerate(ms):
        assert text[o:o + len(t)] == t, (i, name)
        o += len(t)


@pytest.mark.parametrize("res", [0, 1, 2, 3])
def test_ring_sweep_on_device(res):
    """the third block's header on every byte around the ring_advance and ring_reset edges, the payload at in_off = res mod 4"""
    fam = DC.ring_sweep()
    members = [m for m, _ in fam.values()]
    pads = DC.sweep_pads(members, res)
    assert all(o % 4 == res for o in DC.payload_offsets(members, pads))
    text, trunc = device_text(members, pads)
    assert not trunc
    o = 0
    for name, (_, t) in fam.items():
        assert text[o:o + len(t)] == t, name
        o += len(t)
    assert o == len(text)


@pytest.mark.parametrize("name", list(DC.crafted_damage()))
def test_crafted_damage_truncates(name):
    good = [DC.grid()["grid_d64"], DC.one_dist()["one_dist_sym3"], DC.ladder_family()["ladder_order1_p284_1"], DC.mixed()["mixed_stored1025"],
            DC.no_dist()["no_dist"]]
    bad = DC.crafted_damage()[name][0]
    text, trunc = device_text([m for m, _ in good[:3]] + [bad] + [m for m, _ in good[3:]])
    assert trunc and text == b"".join(t for _, t in good[:3])


@pytest.fixture(scope="module")
def crafted_file(tmp_path_factory):
    data, fq, members = DC.crafted_fastq_file(GUIDES)
    path = tmp_path_factory.mktemp("craft") / "crafted.fastq.gz"
    path.write_bytes(data)
    return path, fq.count(b"\n") // 4


@pytest.mark.parametrize("chunk", ["65536", None])
def test_count_file_crafted_members(crafted_file, monkeypatch, capfd, chunk):
    """f2q_count_file with F2Q_DEVICE_INFLATE=1 and without it, on a FASTQ file whose members the craft writer wrote:
    greedy tokens in fixed, stored and ladder-coded blocks, members cut at arbitrary bytes"""
    path, n_reads = crafted_file
    assert n_reads == 3000
    for name in ("m1", "ec"):
        res = check_same(path, KWS[name], monkeypatch, capfd, {"F2Q_FILE_CHUNK": chunk} if chunk else {})
        assert not res[4] and res[3] == n_reads
