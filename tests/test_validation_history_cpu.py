"""CPU: validation.EpochHistory and validation.summarise -- the host half of the validation step: the history dict under the reference's
key names (metrics/train_loss_and_metrics_tracker.py:16-47, :215-265), its pickle, the decision rule (:267-273) and the checkpoint dict
(train/train_synthetic_otf_rendering.py:369-375).  No GPU, no library call."""
import pickle

import numpy as np
import pytest
import torch

import straps_amd
from straps_amd import checkpoint_utils
from straps_amd.metrics import BatchMetrics
from straps_amd.validation import ACC_SLOTS, PER_SAMPLE, EpochHistory, summarise

LOSSES = ['verts', 'shape_params', 'pose_params', 'joints2D', 'joints3D']
METRICS = ['pves', 'pves_sc', 'pves_pa', 'pve-ts', 'pve-ts_sc', 'mpjpes', 'mpjpes_sc', 'mpjpes_pa', 'pose_mses', 'shape_mses', 'joints2D_l2es']
KERNEL_TASKS = ('verts', 'joints2D', 'joints3D', 'shape_params', 'pose_params')
# the reference's 36 history keys
REFERENCE_KEYS = (['train_losses', 'val_losses'] + [s + '_' + t + '_losses' for t in LOSSES for s in ('train', 'val')] +
                  [s + '_' + m for m in METRICS + ['pve-ts_pa'] for s in ('train', 'val')])


def _acc(seed, n):
    """a hand-made accumulator: sums as straps_val_head leaves them after n samples"""
    a = np.random.RandomState(seed).uniform(1.0, 100.0, ACC_SLOTS)
    a[23] = n
    return a


def test_summarise_divides_by_the_trackers_normalisers():
    a = _acc(1, 6)
    s = summarise(a)
    assert s['num_samples'] == 6 and s['losses'] == a[0] / 6
    for k, t in enumerate(KERNEL_TASKS):
        assert s[t + '_losses'] == a[1 + k] / 6
    for k, m in enumerate(BatchMetrics.KEYS):
        assert s[m] == a[12 + k] / (6 * PER_SAMPLE[m])
    assert PER_SAMPLE == {'pves': 6890, 'pves_sc': 6890, 'pves_pa': 6890, 'pve-ts': 6890, 'pve-ts_sc': 6890, 'mpjpes': 14, 'mpjpes_sc': 14,
                          'mpjpes_pa': 14, 'shape_mses': 10, 'pose_mses': 216, 'joints2D_l2es': 17}
    with pytest.raises(RuntimeError):
        summarise(np.zeros(ACC_SLOTS))
    with pytest.raises(ValueError):
        summarise(np.zeros(5))


def test_update_per_epoch_appends_under_the_reference_key_names(tmp_path):
    log = str(tmp_path / 'log.pkl')
    h = EpochHistory(LOSSES, METRICS, log)
    assert sorted(h.history) == sorted(REFERENCE_KEYS) and all(v == [] for v in h.history.values())
    ta, va = _acc(2, 8), _acc(3, 6)
    h.update_per_epoch(summarise(ta), summarise(va))
    for split, a, n in (('train', ta, 8), ('val', va, 6)):
        assert h.history[split + '_losses'] == [a[0] / n]
        for k, t in enumerate(KERNEL_TASKS):
            assert h.history['%s_%s_losses' % (split, t)] == [a[1 + k] / n]
        for k, m in enumerate(BatchMetrics.KEYS):
            assert h.history[split + '_' + m] == [a[12 + k] / (n * PER_SAMPLE[m])]
        assert h.history[split + '_pve-ts_pa'] == [0.0]                 # never computed: 0.0, one entry per epoch all the same
    # what is not tracked, and what a summary does not hold, is 0.0
    h2 = EpochHistory(['verts'], ['pves_pa', 'mpjpes_pa'], None)
    h2.update_per_epoch(None, summarise(va))
    assert h2.history['train_losses'] == [0.0] and h2.history['val_losses'] == [va[0] / 6]
    assert h2.history['val_verts_losses'] == [va[1] / 6] and h2.history['val_joints2D_losses'] == [0.0]
    assert h2.history['val_pves_pa'] == [va[14] / (6 * 6890)] and h2.history['val_pves'] == [0.0] and h2.history['train_pves_pa'] == [0.0]
    assert all(len(v) == 1 for v in h2.history.values())
    with pytest.raises(ValueError):
        EpochHistory(['verts'], ['pck'], None)


def test_pickle_round_trip_and_resume(tmp_path):
    log = str(tmp_path / 'log.pkl')
    h = EpochHistory(LOSSES, METRICS, log)
    for e in range(3):
        h.update_per_epoch(summarise(_acc(10 + e, 8)), summarise(_acc(20 + e, 6)))
    with open(log, 'rb') as f:
        on_disk = pickle.load(f)
    assert type(on_disk) is dict and on_disk == h.history and all(type(x) is float for v in on_disk.values() for x in v)
    # resume after epoch 2: the lists are cut to current_epoch and continued
    r = EpochHistory(LOSSES, METRICS, log, load_logs=True, current_epoch=2)
    assert all(len(v) == 2 for v in r.history.values()) and r.history['val_pves_pa'] == h.history['val_pves_pa'][:2]
    r.update_per_epoch(summarise(_acc(12, 8)), summarise(_acc(22, 6)))
    assert r.history == h.history
    # a log that lacks keys (an older run) is filled with zeros; one that is too short is refused
    del on_disk['val_pve-ts_sc'], on_disk['train_joints3D_losses']
    old = str(tmp_path / 'old.pkl')
    with open(old, 'wb') as f:
        pickle.dump(on_disk, f)
    r2 = EpochHistory(LOSSES, METRICS, old, load_logs=True, current_epoch=3)
    assert r2.history['val_pve-ts_sc'] == [0.0] * 3 and r2.history['train_joints3D_losses'] == [0.0] * 3 and r2.history['val_pves'] == h.history['val_pves']
    with pytest.raises(ValueError):
        EpochHistory(LOSSES, METRICS, old, load_logs=True, current_epoch=4)


def test_decision_rule():
    h = EpochHistory(LOSSES, METRICS, None)
    save = ['pves_pa', 'mpjpes_pa']
    va = _acc(30, 6)
    h.update_per_epoch(None, summarise(va))
    best = {m: np.inf for m in save}
    assert h.determine_save_model_weights_this_epoch(save, best)                     # the first epoch against inf
    best = {m: h.history['val_' + m][-1] for m in save}                             # train loop :358-359
    assert best == {'pves_pa': va[14] / (6 * 6890), 'mpjpes_pa': va[19] / (6 * 14)}
    h.update_per_epoch(None, summarise(va))
    assert h.determine_save_model_weights_this_epoch(save, best)                     # equal to the best: saves
    worse = va.copy()
    worse[19] = np.nextafter(va[19], np.inf) * (1 + 1e-12)                           # one metric strictly greater, the other smaller
    worse[14] = 0.5 * va[14]
    h.update_per_epoch(None, summarise(worse))
    assert h.history['val_mpjpes_pa'][-1] > best['mpjpes_pa'] and h.history['val_pves_pa'][-1] < best['pves_pa']
    assert not h.determine_save_model_weights_this_epoch(save, best)
    assert h.determine_save_model_weights_this_epoch(['pves_pa'], best)              # only the metrics asked for decide
    better = va.copy()
    better[[14, 19]] *= 0.9
    h.update_per_epoch(None, summarise(better))
    assert h.determine_save_model_weights_this_epoch(save, best)


def test_checkpoint_dict_has_the_reference_keys_and_loads(tmp_path):
    torch.manual_seed(0)
    reg = straps_amd.SingleInputRegressor(18, 18, 3, mean_params=straps_amd.synthetic_mean_params(0))
    crit = straps_amd.HomoscedasticUncertaintyWeightedMultiTaskLoss(LOSSES, init_loss_weights={k: 1.0 for k in LOSSES})
    opt = torch.optim.Adam(list(reg.parameters()) + list(crit.parameters()), lr=1e-4)
    best_wts = {k: v.detach().clone() for k, v in reg.state_dict().items()}
    best = {'pves_pa': 0.07, 'mpjpes_pa': 0.05}
    ck = EpochHistory.checkpoint_dict(4, reg, opt, crit, best_epoch=3, best_epoch_val_metrics=best, best_model_wts=best_wts)
    assert tuple(ck) == checkpoint_utils.CHECKPOINT_KEYS and len(ck) == 7
    assert ck['epoch'] == 4 and ck['best_epoch'] == 3 and ck['best_epoch_val_metrics'] == best and ck['best_model_state_dict'] is best_wts
    path = str(tmp_path / 'model_epoch4.tar')
    torch.save(ck, path)
    back = checkpoint_utils.load_checkpoint(path)
    epoch, best_epoch, wts, best_back = checkpoint_utils.load_training_info_from_checkpoint(back, ['pves_pa', 'mpjpes_pa'])
    assert (epoch, best_epoch, best_back) == (5, 3, best)
    reg.load_state_dict(wts)
    assert all(torch.equal(v, best_wts[k]) for k, v in back['model_state_dict'].items())
