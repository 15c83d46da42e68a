"""The bit-31 forms of the register-resident flooding kernel's single-bit
bookkeeping (ms_flood_qc.h with QLDPC_QC_S31) restated in
NumPy on uint32 and compared with the bit-0 forms they replace, for every
combination of sign word, parity word, syndrome bit and check block B.

  bit-0 forms                               bit-31 forms
  synb = (synreg >> B) & 1                  s31 = synreg << (31 - B)
  npm = ((sh >> 31) ^ synb) << 31           npm = (sh ^ s31) & 0x80000000
  unsat |= (ph >> 31) ^ synb; unsat != 0    acc |= ph ^ s31; bit 31 of acc
  parity: ph = synb; ph ^= hw >> c; ph & 1  ph = s31; ph ^= hw << (31 - c); bit 31
"""
import numpy as np
import pytest

MB = 15                                    # check blocks of an LP118_0 half
TOP = np.uint32(0x80000000)


def _words(seed, count):
    """Random words with both values of bit 31 and of every low bit, plus the
    corner words."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([w, np.array([0, 1, 0x7fffffff, 0x80000000, 0x80000001, 0xffffffff], np.uint32)])


@pytest.fixture(scope="module")
def grid():
    """(sh, ph, synreg) over the product of sign words, parity words and
    syndrome registers; every syndrome bit of every block takes both values
    against every (sign bit, parity bit) pair."""
    sh, ph, syn = np.meshgrid(_words(1, 26), _words(2, 26), _words(3, 58) & np.uint32((1 << MB) - 1), indexing="ij")
    for a in (sh, ph, syn):
        a.setflags(write=False)
    return sh.ravel(), ph.ravel(), syn.ravel()


@pytest.mark.parametrize("B", range(MB))
def test_sign_word_and_unsat_bit(grid, B):
    sh, ph, synreg = grid
    synb = (synreg >> np.uint32(B)) & np.uint32(1)
    s31 = synreg << np.uint32(31 - B)
    assert set(np.unique(synb).tolist()) == {0, 1}
    assert np.array_equal(s31 >> np.uint32(31), synb)
    npm0 = ((sh >> np.uint32(31)) ^ synb) << np.uint32(31)
    npm31 = (sh ^ s31) & TOP
    assert np.array_equal(npm0, npm31)
    unsat0 = (ph >> np.uint32(31)) ^ synb
    unsat31 = ph ^ s31
    assert np.array_equal(unsat0 != 0, (unsat31 & TOP) != 0)
    assert np.array_equal(unsat0 != 0, unsat31.view(np.int32) < 0)      # the kernel's signed compare


def test_unsat_accumulated_over_the_blocks_of_a_row(grid):
    """The stop test ORs the blocks' words: bit 31 of the OR of ph_B ^ s31_B is
    set exactly where some block's bit-0 word is non-zero, whatever the lower
    bits of s31 (other blocks' syndrome bits) hold."""
    _, _, synreg = grid
    rng = np.random.default_rng(4)
    acc0 = np.zeros(synreg.shape, np.uint32)
    acc31 = np.zeros(synreg.shape, np.uint32)
    for B in range(MB):
        # parity words that agree with the syndrome bit in most blocks, so that both outcomes occur
        ph = rng.integers(0, 1 << 31, synreg.shape, dtype=np.uint64).astype(np.uint32)
        agree = rng.random(synreg.shape) < 0.97
        bit = ((synreg >> np.uint32(B)) & np.uint32(1)) ^ (~agree).astype(np.uint32)
        ph |= bit << np.uint32(31)
        acc0 |= (ph >> np.uint32(31)) ^ ((synreg >> np.uint32(B)) & np.uint32(1))
        acc31 |= ph ^ (synreg << np.uint32(31 - B))
    want = acc0 != 0
    assert want.any() and not want.all()
    assert np.array_equal(want, acc31.view(np.int32) < 0)


@pytest.mark.parametrize("B", range(MB))
def test_max_iter_parity_word(grid, B):
    """qc_parity: the hard decisions of variable block c sit at bit c & 31 of a
    packed word; eight edges with assorted c, the syndrome bit of block B."""
    hw0, hw1, synreg = grid
    hw = (hw0, hw1)
    cols = (0, 1, 7, 30, 31, 32, 33, 2 * B + 3)           # variable blocks 0 .. 33
    synb = (synreg >> np.uint32(B)) & np.uint32(1)
    p0 = synb.copy()
    p31 = synreg << np.uint32(31 - B)
    for c in cols:
        p0 ^= hw[c >> 5] >> np.uint32(c & 31)
        p31 ^= hw[c >> 5] << np.uint32(31 - (c & 31))
    p0 &= np.uint32(1)
    assert set(np.unique(p0).tolist()) == {0, 1}
    assert np.array_equal(p0, p31 >> np.uint32(31))
    assert np.array_equal(p0 != 0, p31.view(np.int32) < 0)
