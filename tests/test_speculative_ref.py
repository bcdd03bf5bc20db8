"""CPU: the accept rule of speculative decoding (tests/spec_ref.py) on hand-written cases -- what the GPU tests hold k_spec_accept to."""
import numpy as np

import spec_ref

NI = -np.inf


def test_row_argmax_takes_the_lowest_index_on_ties():
    lg = np.array([[1.0, 3.0, 3.0, 2.0],      # two equal maxima
                   [5.0, 1.0, 5.0, 5.0],      # three, one at index 0
                   [0.0, 7.0, 1.0, 7.0],      # one at V - 1
                   [NI, NI, NI, NI],          # all -inf
                   [NI, -1.0, NI, -1.0]], dtype=np.float32)
    assert spec_ref.row_argmax(lg).tolist() == [1, 0, 1, 0, 1]


def test_prefix_match_and_the_correction_token():
    am = np.array([4, 9, 2, 7])
    assert spec_ref.accept(am, [4, 9, 2])[0] == 3 and spec_ref.accept(am, [4, 9, 2])[1].tolist() == [4, 9, 2, 7]      # everything accepted: bonus token
    assert spec_ref.accept(am, [4, 9, 5])[0] == 2 and spec_ref.accept(am, [4, 9, 5])[1].tolist() == [4, 9, 2]
    assert spec_ref.accept(am, [4, 1, 2])[0] == 1 and spec_ref.accept(am, [4, 1, 2])[1].tolist() == [4, 9]            # a later agreement does not count
    assert spec_ref.accept(am, [0, 9, 2])[0] == 0 and spec_ref.accept(am, [0, 9, 2])[1].tolist() == [4]
    assert spec_ref.accept(np.array([6]), [])[0] == 0 and spec_ref.accept(np.array([6]), [])[1].tolist() == [6]       # R = 1: a plain decode step


def test_record_layout():
    lg = np.zeros((3, 5), dtype=np.float32)
    lg[0, 2] = lg[1, 4] = lg[2, 1] = 1.0
    assert spec_ref.record(lg, [2, 4]).tolist() == [2, 2, 4, 1]
    assert spec_ref.record(lg, [2, 0]).tolist() == [1, 2, 4, -1]
    assert spec_ref.record(lg, [3, 4]).tolist() == [0, 2, -1, -1]
    assert spec_ref.record(lg[:1], []).tolist() == [0, 2]
