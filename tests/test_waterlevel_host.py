"""Host side of the water-level estimator (``vfloodnet_amd.waterlevel``, no GPU): the Gaussian smoothing against scipy, the
carry-forward / NaN rule of reference_tracking.py:190-206, ``waterlevel.csv`` against pandas, the record files and the
calibration default of the command line."""
import argparse

import numpy as np
import pytest

from vfloodnet_amd import waterlevel as WL


def _series():
    rng = np.random.RandomState(7)
    out = []
    for n in (1, 5, 40):
        x = rng.uniform(0, 60, n)
        out.append(x)
        for nan_at in ([0], [n - 1], [n // 2], [0, n - 1]):
            y = x.copy()
            y[nan_at] = np.nan
            out.append(y)
    z = rng.uniform(0, 60, 40)
    z[11:15] = np.nan                      # a NaN run in the middle
    out.append(z)
    z = rng.uniform(0, 60, 40)
    z[:3] = np.nan
    z[-2:] = np.nan
    out.append(z)
    return out


@pytest.mark.parametrize('x', _series(), ids=lambda x: f'n{x.size}_nan{int(np.isnan(x).sum())}_{int(np.isnan(x[0]))}{int(np.isnan(x[-1]))}')
def test_smooth_equals_scipy_gaussian_filter1d(x):
    from scipy.ndimage import gaussian_filter1d
    want = gaussian_filter1d(x, sigma=2, mode='nearest')
    got = WL.smooth(x)
    assert got.dtype == np.float64 and got.shape == x.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= 1e-12


def test_nan_spreads_eight_frames_either_way():
    x = np.full(40, 3.0)
    x[20] = np.nan
    assert np.flatnonzero(np.isnan(WL.smooth(x))).tolist() == list(range(12, 29))


def test_carry_forward_and_nan_rule():
    nan = np.nan
    #            ref 0: nothing at frame 0 -> 0; hit; kept; offset 1 -> NaN; NaN carried over -1; recovery
    log = np.array([[-1, 5],
                    [7, -1],
                    [-1, 1],
                    [1, -1],
                    [-1, -1],
                    [4, 9],
                    [-1, 2]], np.int32)
    want = np.array([[0, 5], [7, 5], [7, nan], [nan, nan], [nan, nan], [4, 9], [4, 2]], np.float64)
    got = WL.levels_from_offsets(log)
    assert got.dtype == np.float64
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(WL.nanmean_rows(want), np.array([2.5, 6, 7, nan, nan, 6.5, 3]), equal_nan=True)


def _frame(names, levels):
    pd = pytest.importorskip('pandas')
    from datetime import datetime
    idx = []
    for n in names:
        try:
            idx.append(datetime.strptime(n, '%Y-%m-%d-%H-%M-%S'))
        except ValueError:
            idx.append(n)
    df = pd.DataFrame(levels, index=idx, columns=[f'est_ref{i}_px' for i in range(levels.shape[1])])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        df['est_avg_px'] = np.nanmean(levels, axis=1)
    return df


CSV_CASES = {
    'timestamps': ['2021-09-01-12-00-00', '2021-09-01-12-00-30', '2021-09-01-12-01-00', '2021-09-02-00-00-00'],
    'midnights': ['2021-09-01-00-00-00', '2021-09-02-00-00-00', '2021-09-03-00-00-00', '2021-09-04-00-00-00'],
    'mixed_names': ['2021-09-01-12-00-00', '00001', 'frame,with "quotes"', '2021-09-01-12-01-00'],
}


@pytest.mark.parametrize('case', sorted(CSV_CASES))
def test_csv_bytes_equal_pandas(case, tmp_path):
    names = CSV_CASES[case]
    levels = np.array([[12.5, 3.0], [np.nan, np.nan], [1e-5, 123456789.125], [0.1 + 0.2, np.nan]], np.float64)
    avg = WL.nanmean_rows(levels)
    want = _frame(names, levels).to_csv().encode('utf-8')
    assert WL.csv_bytes(names, levels, avg) == want
    assert b'\n2021-09-0' in want and b',,,\n' in want              # an all-NaN row is three empty fields


def test_load_records_and_keypoints(tmp_path):
    rec = tmp_path / 'groundtruth'
    (rec / 'one').mkdir(parents=True)
    (rec / 'two').mkdir()
    homo = np.array([[1.02, 0.05, -3.0], [0.01, 0.98, 2.0], [1e-4, 2e-4, 1.0]])
    np.savetxt(str(rec / 'one' / 'homo_mat.txt'), homo, '%.4f')                       # as reference_tracking.py:78 writes it
    np.savetxt(str(rec / 'one' / 'ref_bbox.txt'), np.array([(101, 52, 31, 77)]), '%.4f')      # :102, one reference
    np.savetxt(str(rec / 'two' / 'ref_bbox.txt'), np.array([(10.9, 5.2, 9.7, 11.0), (40, 8, 7, 9)]), '%.4f')
    m, boxes = WL.load_records(str(rec), 'one')
    assert m.shape == (3, 3) and m.dtype == np.float64 and np.array_equal(m, np.round(homo, 4))
    assert boxes.tolist() == [[101, 52, 31, 77]]
    m, boxes = WL.load_records(str(rec), 'two', calib=False)
    assert m is None and boxes.tolist() == [[10, 5, 9, 11], [40, 8, 7, 9]]            # astype(int): truncation
    assert WL.keypoints(boxes).tolist() == [[int(10 + 9 / 2), 16], [int(40 + 7 / 2), 17]] == [[14, 16], [43, 17]]
    assert WL.keypoints([101, 52, 31, 77]).tolist() == [[116, 129]]
    with pytest.raises(FileNotFoundError, match='homo_mat.txt'):
        WL.load_records(str(rec), 'two')
    with pytest.raises(FileNotFoundError, match='ref_bbox.txt'):
        WL.load_records(str(rec), 'three', calib=False)


def test_cli_calibration_default_follows_the_test_name():
    from vfloodnet_amd import est_waterlevel as E
    ns = lambda name, **kw: argparse.Namespace(test_name=name, no_calib=False, homo_mat=None, **kw)
    assert E.use_calibration(ns('houston_buffalo')) is False
    assert E.use_calibration(ns('LSU_20200423')) is False
    assert E.use_calibration(ns('boston_harbor')) is True
    assert E.use_calibration(ns('my_clip')) is True
    assert E.use_calibration(argparse.Namespace(test_name='my_clip', no_calib=True, homo_mat='h.txt')) is False
    assert E.use_calibration(argparse.Namespace(test_name='houston_buffalo', no_calib=False, homo_mat='h.txt')) is True
    args = E.get_parser(['--test-name', 'houston_x', '--test-path', 'frames', '--opt', 'ref'])
    assert args.out_dir == 'output/waterlevel' and args.viz is True and E.use_calibration(args) is False
    with pytest.raises(NotImplementedError):
        E.main(E.get_parser(['--test-name', 'x', '--test-path', 'frames', '--opt', 'people']))


def test_smooth_follows_scipys_summation_order():
    """The CSV holds shortest-repr floats, so ``waterlevel.csv`` equals the reference's only if the filter agrees to the bit."""
    from scipy.ndimage import gaussian_filter1d
    rng = np.random.RandomState(3)
    for i in range(200):
        x = rng.randint(0, 300, rng.randint(1, 60)).astype(np.float64) if i % 2 else rng.uniform(0, 300, rng.randint(1, 60))
        assert np.array_equal(WL.smooth(x), gaussian_filter1d(x, sigma=2, mode='nearest'))
