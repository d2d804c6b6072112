"""Writes tests/golden/bitnet/bitnet_packed_ref.npz: the packed ternary format as its authors' code produces it,
``transformers.integrations.bitnet.pack_weights`` (needs the transformers package; the tests that read the file do not).
(A directory of its own: every tests/golden/*.npz is a qgemm case of the oracle and emulation tests.)

  ternary [64][32] int8   a seeded matrix of {-1, 0, 1}
  packed  [16][32] uint8  pack_weights(ternary)
  ex_ternary [8][2] int8, ex_packed [2][2] uint8   the worked example of unpack_weights' docstring: pack_weights of the printed output
                                                   must give the printed input, which the script asserts before it writes anything

Run from the repository root:  python tests/golden/make_bitnet_packed_ref.py
"""
import os

import numpy as np
import torch
from transformers.integrations.bitnet import pack_weights

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ternary = np.random.default_rng(20260223).integers(-1, 2, size=(64, 32)).astype(np.int8)
    packed = pack_weights(torch.from_numpy(ternary.copy())).numpy()          # (pack_weights adds 1 to its argument in place)
    ex_ternary = np.array([[0, -1], [-1, 1], [-1, 1], [-1, 1], [1, 0], [0, -1], [1, -1], [1, -1]], np.int8)
    ex_packed = pack_weights(torch.from_numpy(ex_ternary.copy())).numpy()
    assert np.array_equal(ex_packed, np.array([[0b10100001, 0b00011000], [0b10010000, 0b00001010]], np.uint8)), ex_packed
    assert packed.dtype == np.uint8 and packed.shape == (16, 32) and set(np.unique(ternary)) == {-1, 0, 1}
    os.makedirs(os.path.join(HERE, "bitnet"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "bitnet", "bitnet_packed_ref.npz"), ternary=ternary, packed=packed, ex_ternary=ex_ternary, ex_packed=ex_packed)


if __name__ == "__main__":
    main()
