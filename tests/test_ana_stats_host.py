"""Per-event, per-class analysis statistics, host side (no GPU): the three appended symbols under an unchanged ABI 9, the scratch
query, the derivation of the result dict and of the CSV text from raw counts and sums (ssnet.class_stats_from_counts,
ana_csv_header, ana_csv_row) against a numpy restatement of the reference's example_scripts/ana_csv.py:67-116, and the ANA_CSV
key."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import uresnet_amd  # noqa: F401
from uresnet_amd import _lib, ssnet_config
from uresnet_amd.ssnet import ana_csv_header, ana_csv_row, class_stats_from_counts

SPAN = 4096           # voxels per workgroup (CSTATS_SPAN)


def test_symbols_appended_under_abi_9(lib):
    assert _lib.ABI_VERSION == 9 and lib.ursn_abi_version() == 9
    for name in ("ursn_class_stats", "ursn_class_stats_scratch_bytes", "ursn_infer_stats"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_scratch_query(lib):
    q = lib.ursn_class_stats_scratch_bytes
    sizes = [1, 5, SPAN - 1, SPAN, SPAN + 1, 192 ** 3, 256 ** 3, 2 ** 31 - 1]
    for n in (1, 3, 65535):
        for c in range(1, 9):
            got = [q(n, v, c) for v in sizes]
            assert all(g > 0 for g in got) and got == sorted(got), (n, c)
            assert q(n, SPAN, c) < q(n, SPAN + 1, c)                      # one more span
    # per event and span: 2 NC doubles and NC * NC + 4 uint32 counts, classes padded to NC = 4 | 8
    per = {4: 2 * 4 * 8 + (16 + 4) * 4, 8: 2 * 8 * 8 + (64 + 4) * 4}
    assert q(1, 1, 3) == per[4] and q(1, 1, 5) == per[8]
    assert q(4, 192 ** 3, 3) == 4 * -(-192 ** 3 // SPAN) * per[4]
    for n, v, c in ((0, 64, 3), (-1, 64, 3), (65536, 64, 3), (1, 0, 3), (1, -5, 3), (1, 2 ** 31, 3), (1, 2 ** 40, 3),
                    (1, 64, 0), (1, 64, 9), (1, 64, -1)):
        assert q(n, v, c) == 0, (n, v, c)


# ---- the reference's loop, restated -----------------------------------------------------------------------------------------
def reference_rows(entries, softmax_batch, label_batch, num_class):
    """example_scripts/ana_csv.py:67-116 in Python 3: the numbers of each event's row and the row's text."""
    rows, texts = [], []
    for index in range(len(softmax_batch)):
        entry, softmax, label = entries[index], softmax_batch[index], np.squeeze(label_batch[index])
        prediction = np.argmax(softmax, axis=-1).astype(np.float32)
        acc_all = float((prediction == label).sum()) / prediction.size
        nonzero_px = np.where(label > 0)
        nonzero_prediction, nonzero_label = prediction[nonzero_px], label[nonzero_px]
        acc_nonzero = (float((nonzero_prediction == nonzero_label).sum()) / nonzero_prediction.size
                       if nonzero_prediction.size else float('nan'))   # the reference divides by zero here
        text = '%d,%g,%g' % (entry, acc_all, acc_nonzero)
        row = {'acc_all': acc_all, 'acc_nonzero': acc_nonzero, 'npx': [], 'acc': [], 'mean': [], 'std': []}
        for class_label in range(num_class):
            class_mask = np.where(label == class_label)
            npx = label[class_mask].size
            class_acc = class_score_mean = class_score_std = -1.
            if npx:
                class_prediction = prediction[class_mask]
                class_acc = float((class_prediction == class_label).sum()) / npx
                class_score = (softmax[..., class_label])[class_mask]
                class_score_mean = class_score.mean()
                class_score_std = class_score.std()
            text += ',%d,%g,%g,%g' % (npx, class_acc, class_score_mean, class_score_std)
            for k, v in (('npx', npx), ('acc', class_acc), ('mean', class_score_mean), ('std', class_score_std)):
                row[k].append(v)
        rows.append(row)
        texts.append(text + '\n')
    return rows, texts


def raw_counts(softmax_batch, label_batch, num_class):
    """What ursn_class_stats returns for these scores and integer labels: conf, other, fp64 score sums."""
    n, C = len(softmax_batch), num_class
    conf, other = np.zeros((n, C, C), np.int64), np.zeros((n, 2), np.int64)
    ssum, ssq = np.zeros((n, C)), np.zeros((n, C))
    for e in range(n):
        sm, lab = softmax_batch[e].reshape(-1, C), label_batch[e].reshape(-1)
        pred, t = sm.argmax(axis=1), lab.astype(np.int64)
        ok = (t >= 0) & (t < C)
        np.add.at(conf[e], (t[ok], pred[ok]), 1)
        other[e] = [np.count_nonzero(~ok & (lab > 0)), np.count_nonzero(~ok & ~(lab > 0))]
        for k in range(C):
            s = sm[ok & (t == k), k].astype(np.float64)
            ssum[e, k], ssq[e, k] = s.sum(), (s * s).sum()
    return conf, other, ssum, ssq


def _events(C, shape=(24, 20), seed=11):
    """Scores free of ties by construction (per voxel, class k holds a multiple of 8 plus k, over 1024: exact in fp32 and distinct)
    and labels: all classes / one class absent / no label > 0 / a label == C (counts for acc_nonzero, matches no prediction)."""
    rng = np.random.default_rng(seed)
    n = 4
    sm = ((rng.integers(0, 100, (n,) + shape + (C,)) * 8 + np.arange(C) + 1) / 1024.0).astype(np.float32)
    lab = rng.integers(0, C, (n,) + shape).astype(np.float32)
    if C > 1:
        lab[1][lab[1] == C - 1] = 0.0
    lab[2][:] = 0.0
    lab[3].reshape(-1)[::7] = float(C)
    return sm, lab


@pytest.mark.parametrize("C", [1, 2, 3, 5])
def test_dict_and_csv_text_against_the_reference_loop(C):
    sm, lab = _events(C)
    n = sm.shape[0]
    entries = [7, 8, 40, 41]
    rows, texts = reference_rows(entries, sm, lab[..., None], C)
    conf, other, ssum, ssq = raw_counts(sm, lab, C)
    st = class_stats_from_counts(conf, other, ssum, ssq)
    assert set(st) == {'conf', 'other', 'npx', 'acc_class', 'score_mean', 'score_std', 'acc_all', 'acc_nonzero_label',
                       'acc_nonzero_data'}
    assert st['conf'].dtype == np.int64 and st['conf'].shape == (n, C, C) and st['npx'].shape == (n, C)
    assert np.isnan(st['acc_nonzero_data']).all()
    if C > 1:
        assert st['npx'][1, C - 1] == 0 and st['acc_class'][1, C - 1] == -1.0 and st['score_std'][1, C - 1] == -1.0
    assert np.isnan(st['acc_nonzero_label'][2]) and np.isnan(rows[2]['acc_nonzero'])
    assert st['other'][3, 0] > 0
    for e in range(n):
        assert list(st['npx'][e]) == rows[e]['npx']
        assert st['acc_all'][e] == rows[e]['acc_all']
        if np.isnan(rows[e]['acc_nonzero']):                      # no label > 0 in the event
            assert np.isnan(st['acc_nonzero_label'][e])
        else:
            assert st['acc_nonzero_label'][e] == rows[e]['acc_nonzero']
        assert list(st['acc_class'][e]) == rows[e]['acc']
        np.testing.assert_allclose(st['score_mean'][e], np.asarray(rows[e]['mean'], np.float64), rtol=1e-6)
        np.testing.assert_allclose(st['score_std'][e], np.asarray(rows[e]['std'], np.float64), rtol=1e-5, atol=1e-7)
        assert ana_csv_row(entries[e], st, e) == texts[e]
    assert ana_csv_header(C) == 'entry,acc_all,acc_nonzero' + ''.join(
        ',npx_class%d,acc_class%d,mean_softmax_class%d,std_softmax_class%d' % (i, i, i, i) for i in range(C)) + '\n'
    assert ana_csv_header(C).count(',') == texts[0].count(',')


def test_acc_nonzero_data_from_the_nonzero_counts():
    conf = np.array([[[3, 1], [0, 4]], [[8, 0], [0, 0]]])
    st = class_stats_from_counts(conf, np.zeros((2, 2), np.int64), np.ones((2, 2)), np.ones((2, 2)), nonzero=[[4, 3], [0, 0]])
    assert st['acc_nonzero_data'][0] == 0.75 and np.isnan(st['acc_nonzero_data'][1])
    assert st['acc_all'][0] == 7 / 8 and st['acc_nonzero_label'][0] == 1.0 and np.isnan(st['acc_nonzero_label'][1])


def test_ana_csv_key(tmp_path):
    assert ssnet_config().ANA_CSV == ''
    p = tmp_path / "a.cfg"
    p.write_text("ANA_CSV 'out/ana.csv'\n")
    c = ssnet_config()
    with redirect_stdout(io.StringIO()):
        c.override(str(p))
    assert c.ANA_CSV == 'out/ana.csv' and ssnet_config().ANA_CSV == ''
    bad = tmp_path / "b.cfg"
    bad.write_text("ANA_CSV True\n")
    with redirect_stdout(io.StringIO()), pytest.raises(TypeError):
        ssnet_config().override(str(bad))
