"""K5 (least_rotation.hip) on the inputs of tests/k5_shapes.py: index, rotated bytes and seqhash equal the CPU oracle
exactly (integers and bytes: no tolerance).  tests/test_k5_shapes_cpu.py asserts the inputs' properties.

  forward strand   polyhip_least_rotation_batch on every family member and its reverse complement
  second strand    HashBatch(circular, double-stranded): the search on the reverse-complement view (`strand == 1` of the
                   wave kernel, `rc = 1` / RcView of the workgroup kernels) decides the hash of every input whose second
                   strand is the smaller one -- one of t and revcomp(t), and both are here; the single-stranded hash of
                   the same inputs tells the strands apart
  many sequences   40,000 short ones: a wave takes several in turn, a workgroup works through chunks of four marks and goes
                   round its grid more than once

POLYHIP_K5_WAVE_MAX moves the boundary between the wave kernel and the workgroup kernels: unset = 7,168 bytes, 0 = every
sequence of more than 8 bytes through the workgroup kernels, 100 / 32768 = other splits.  The size-one inputs (up to
7,168 bytes) so pass through the wave kernel and the LDS workgroup kernel, the size-two inputs (122,857 bytes and more)
through the global-memory kernel under every setting."""
import functools
import time

import numpy as np
import pytest

import k5_shapes as ks
import oracle as orc

pytestmark = pytest.mark.gpu

WAVE_MAX = [None, "0", "100", "32768"]
N_MANY = 40_000


@pytest.fixture(scope="module")
def sh():
    from poly_amd import seqhash
    return seqhash


def _set_wave_max(monkeypatch, wave_max):
    if wave_max is None:
        monkeypatch.delenv("POLYHIP_K5_WAVE_MAX", raising=False)
    else:
        monkeypatch.setenv("POLYHIP_K5_WAVE_MAX", wave_max)


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


# ---- the oracle's answers, computed once per batch and left alone
@functools.lru_cache(maxsize=None)
def _batches(size):
    return ks.batches(size)


@functools.lru_cache(maxsize=None)
def _want_rotation(key):
    seqs = _seqs(key)
    return (np.array([orc.booth_least_rotation(s) for s in seqs], np.uint64),
            np.frombuffer(b"".join(orc.rotate_sequence(s) for s in seqs), np.uint8))


@functools.lru_cache(maxsize=None)
def _want_hash(key, ds):
    return tuple(orc.seqhash(s, "DNA", True, ds) for s in _seqs(key))


def _seqs(key):
    return ks.many_short(N_MANY)[0] if key == "many" else _batches(key[0])[key[1]][1]


def _names(key):
    return None if key == "many" else _batches(key[0])[key[1]][0]


def _keys(size):
    return [(size, b) for b in range(len(_batches(size)))]


def _check_rotation(key, rot, out):
    seqs, names = _seqs(key), _names(key)
    want_rot, want_out = _want_rotation(key)
    bad = np.flatnonzero(np.asarray(rot, np.uint64)[:len(seqs)] != want_rot)
    assert len(bad) == 0, [(int(i), names[i] if names else len(seqs[i]), int(rot[i]), int(want_rot[i])) for i in bad[:5]]
    if not np.array_equal(out[:len(want_out)], want_out):
        offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        at = int(np.flatnonzero(out[:len(want_out)] != want_out)[0])
        i = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError(("rotated bytes", i, names[i] if names else len(seqs[i]), at - int(offs[i])))


def _check_hash(key, ds, got):
    seqs, names = _seqs(key), _names(key)
    want = _want_hash(key, ds)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), [(i, names[i] if names else seqs[i][:40], "double" if ds else "single") for i in bad[:5]]


# ---- a. forward strand --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave_max", WAVE_MAX)
@pytest.mark.parametrize("size", [1, 2])
def test_forward_strand(sh, monkeypatch, size, wave_max):
    """index = Booth's, bytes = RotateSequence's, on every family member and its reverse complement"""
    _set_wave_max(monkeypatch, wave_max)
    for key in _keys(size):
        _want_rotation(key)
        t0 = time.perf_counter()
        buf, offs = _pack(_seqs(key))
        rot, out = sh.least_rotation_batch_packed(buf, offs, True)
        print(f"{_names(key)[0]:18s} {len(_seqs(key)):3d} sequences {1e3 * (time.perf_counter() - t0):8.1f} ms")
        _check_rotation(key, rot, out)


# ---- b. second strand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave_max,fold", [(w, True) for w in WAVE_MAX] + [(None, False)],
                         ids=[f"wave_max={w}" for w in WAVE_MAX] + ["unfolded"])
@pytest.mark.parametrize("size", [1, 2])
def test_second_strand(sh, monkeypatch, size, wave_max, fold):
    """Hash of a circular double-stranded sequence is the hash of the smaller rotated strand: equal to the oracle's for t
    and for revcomp(t), in one of which the second strand's index decides it.  The single-stranded hash of the same batch
    says which strand a failure belongs to.  unfolded (POLYHIP_S2_FOLD=0): the wave kernel stages normalised bytes instead
    of normalising the caller's while it stages them -- the other of its two stagings of the first strand."""
    _set_wave_max(monkeypatch, wave_max)
    if fold:
        monkeypatch.delenv("POLYHIP_S2_FOLD", raising=False)
    else:
        monkeypatch.setenv("POLYHIP_S2_FOLD", "0")
    for key in _keys(size):
        _want_hash(key, True), _want_hash(key, False)
        t0 = time.perf_counter()
        double = sh.HashBatch(list(_seqs(key)), "DNA", True, True)
        single = sh.HashBatch(list(_seqs(key)), "DNA", True, False)
        print(f"{_names(key)[0]:18s} {len(_seqs(key)):3d} sequences {1e3 * (time.perf_counter() - t0):8.1f} ms")
        _check_hash(key, False, single)
        _check_hash(key, True, double)


@pytest.mark.parametrize("wave_max", WAVE_MAX)
@pytest.mark.parametrize("size", [1, 2])
def test_a_full_second_strand_list_behind_a_winning_first_strand(sh, monkeypatch, size, wave_max):
    """inputs whose own strand wins while the other has more than 1,024 candidates, and their reverse complements: one
    double-stranded hash for both, the oracle's; two different single-stranded ones"""
    _set_wave_max(monkeypatch, wave_max)
    picked = ks.forward_wins_full_reverse(size)
    assert picked
    ts = [t for _, t in picked]
    rs = [ks.revcomp(t) for t in ts]
    double = sh.HashBatch(ts + rs, "DNA", True, True)
    single = sh.HashBatch(ts + rs, "DNA", True, False)
    for i, (name, t) in enumerate(picked):
        assert double[i] == double[len(ts) + i] == orc.seqhash(t, "DNA", True, True), name
        assert single[i] != single[len(ts) + i], name
        assert single[i] == orc.seqhash(t, "DNA", True, False) and single[len(ts) + i] == orc.seqhash(rs[i], "DNA", True, False), name


# ---- c. many sequences --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave_max", [None, "0", "100"])
def test_many_sequences(sh, monkeypatch, wave_max):
    """40,000 sequences of 0 to 300 bytes, long and short in turn.  unset: 2,048 workgroups of four waves, every wave takes
    four or five sequences one after another on the same LDS and lists.  0: every sequence of more than 8 bytes is marked,
    a workgroup reads four marks at a time and 1,808 of the 8,192 workgroups come round a second time.  100: the long half
    is marked, two marks in most chunks."""
    _set_wave_max(monkeypatch, wave_max)
    seqs = _seqs("many")
    buf, offs = _pack(seqs)
    rot, out = sh.least_rotation_batch_packed(buf, offs, True)
    _check_rotation("many", rot, out)
    _check_hash("many", True, sh.HashBatch(list(seqs), "DNA", True, True))


def test_many_sequences_on_device_tensors(sh, monkeypatch):
    import torch
    _set_wave_max(monkeypatch, None)
    buf, offs = _pack(_seqs("many"))
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(buf).to(dev)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    rot = torch.full((N_MANY,), -1, dtype=torch.int64, device=dev)
    out = torch.zeros_like(d_seqs)
    sh.least_rotation_batch_dev(d_seqs, d_offs, int(np.diff(offs).max()), rot, out)
    torch.cuda.synchronize()
    _check_rotation("many", rot.cpu().numpy().view(np.uint64), out.cpu().numpy())
