"""Host half of the LIP support (no GPU): the value map of random_hflip.swap_pair and that it leaves the drawn decisions alone
(lib/datasets/tools/gpu_aug.py), DataHelper.prepare_data(want_reverse=True), the permutation of the validation pass, test.flip_swap_pair in
segmentor/tester.py::check_config, and the two configs of configs/lip."""
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIP_PAIRS = [[14, 15], [16, 17], [18, 19]]
LIP_PERM = list(range(14)) + [15, 14, 17, 16, 19, 18]
SIZES = [(83, 61), (473, 473), (160, 96), (40, 33), (473, 473), (64, 48)] * 5


def _cfg(pairs, **data):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    return Configer(config_dict={
        "data": dict({"num_classes": 20}, **data),
        "train": {"data_transformer": {"size_mode": "fix_size", "input_size": [473, 473], "align_method": "only_pad", "pad_mode": "random"}},
        "train_trans": {"trans_seq": ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"],
                        "random_brightness": {"ratio": 1.0, "shift_value": 10}, "resize": {"target_size": [473, 473]},
                        "random_hflip": {"ratio": 0.5, "swap_pair": pairs},
                        "random_resize": {"ratio": 0.7, "method": "random", "scale_range": [0.5, 1.5], "aspect_range": [0.9, 1.1]},
                        "random_crop": {"ratio": 1.0, "crop_size": [473, 473], "method": "random", "allow_outside_center": False}},
        "normalize": {"div_value": 255.0, "mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}})


def test_swap_pair_leaves_the_random_sequence_and_the_records_alone():
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    runs = []
    for pairs in (LIP_PAIRS, [], None):
        t = GPUBatchTransform(_cfg(pairs))
        random.seed(1234)
        params, offsets, target = t.plan_ragged(SIZES)
        runs.append((params, offsets, target, random.getstate()))
    for params, offsets, target, state in runs[1:]:
        assert torch.equal(params, runs[0][0]) and torch.equal(offsets, runs[0][1]) and target == runs[0][2]
        assert state == runs[0][3]                          # the same number of draws: the stream goes on from the same point
    rows = runs[0][0].numpy()
    # the sequence exercises every place a flip can end up in
    assert rows[:, 4].any() and rows[:, 7].any() and rows[:, 12].any() and (rows[:, 2] > 0).any()


def test_swap_table_construction():
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUAugCompose, GPUBatchTransform, swap_table
    assert swap_table([]) is None and swap_table(None) is None
    swap = swap_table(LIP_PAIRS)
    assert swap.dtype == np.uint8 and swap.shape == (256,)
    assert swap[:20].tolist() == LIP_PERM and np.array_equal(swap[20:], np.arange(20, 256))
    # overlapping pairs: the partner in the LAST pair that mentions a value, as the reference's loop over a copy gives
    for pairs in ([[1, 2], [2, 3]], [[2, 3], [1, 2]], [[5, 5], [5, 6]], [(1, 2), (3, 1), (2, 3)]):
        lab = np.arange(256, dtype=np.uint8)
        temp = lab.copy()
        for a, b in pairs:
            lab[temp == a] = b
            lab[temp == b] = a
        assert np.array_equal(swap_table(pairs), lab), pairs
    assert swap_table([[1, 2], [2, 3]])[:5].tolist() == [0, 2, 3, 2, 4]
    for pairs, what in (([[14, 255]], "mentions 255"), ([[255, 3]], "mentions 255"), ([[14, 15, 16]], "two integer label ids"),
                        ([[14]], "two integer label ids"), ([[14, 1.5]], "two integer label ids"), ([["a", 1]], "two integer label ids"),
                        ([[True, 1]], "two integer label ids"), ([[14, 256]], "0..254"), ([[-1, 3]], "0..254"), ([14, 15], "two integer"),
                        ("14,15", "list of")):
        with pytest.raises(ValueError, match=what):
            swap_table(pairs)
        with pytest.raises(ValueError, match=what):
            GPUAugCompose(_cfg(pairs))
    # lut_mirrored = lut o swap; over the identity where there is no label encoding (LIP has none)
    t = GPUBatchTransform(_cfg(LIP_PAIRS))
    assert t.lut is None and t.lut_mirrored.dtype == torch.int16 and t.lut_mirrored.tolist() == swap.tolist()
    ids = [0, 14, 15, 16, 30]
    t = GPUBatchTransform(_cfg([[14, 15], [16, 30]], label_list=ids))
    lut = t.lut.numpy()
    assert [int(lut[i]) for i in ids] == [0, 1, 2, 3, 4]
    assert [int(t.lut_mirrored[i]) for i in ids] == [0, 2, 1, 4, 3] and int(t.lut_mirrored[7]) == 255
    t = GPUBatchTransform(_cfg([[1, 2]], reduce_zero_label=True))
    assert t.lut_mirrored[:4].tolist() == [255, 1, 0, 2]
    assert GPUBatchTransform(_cfg([])).lut_mirrored is None
    # without random_hflip in the sequence the key plays no part
    cfg = _cfg(LIP_PAIRS)
    cfg.get("train_trans")["trans_seq"] = ["resize", "random_crop"]
    assert GPUBatchTransform(cfg).lut_mirrored is None


def test_prepare_data_with_want_reverse():
    from contrastiveseg_amd.segmentor.tools.data_helper import DataHelper

    class _Runner(object):
        @staticmethod
        def device():
            return torch.device("cpu")

    class _Trainer(object):
        module_runner = _Runner()

    helper = DataHelper(None, _Trainer())
    g = torch.Generator().manual_seed(3)
    batch = {"img": torch.randn(2, 3, 4, 5, generator=g), "labelmap": torch.randint(-1, 20, (2, 4, 5), generator=g)}
    (inputs, targets), n = helper.prepare_data(batch)
    assert n == 2 and len(inputs) == 1 and inputs[0] is batch["img"] and targets is batch["labelmap"]
    (inputs, targets, inputs_rev, targets_rev), n = helper.prepare_data(batch, want_reverse=True)
    assert n == 2 and inputs[0] is batch["img"] and targets is batch["labelmap"]
    assert len(inputs_rev) == 1 and inputs_rev[0].shape == (2, 3, 4, 5) and targets_rev.shape == (2, 4, 5)
    assert torch.equal(inputs_rev[0], torch.from_numpy(batch["img"].numpy()[..., ::-1].copy()))
    assert torch.equal(targets_rev, torch.from_numpy(batch["labelmap"].numpy()[..., ::-1].copy()))
    assert torch.equal(torch.cat([inputs[0], inputs_rev[0]], 0)[2:], torch.flip(batch["img"], [3]))


def test_the_validation_permutation_is_the_references_hard_coded_rule():
    from contrastiveseg_amd.segmentor.trainer_contrastive import LIP_SWAP_PAIRS, lip_mirror_perm
    assert [list(p) for p in LIP_SWAP_PAIRS] == LIP_PAIRS
    assert lip_mirror_perm(20) == LIP_PERM
    assert lip_mirror_perm(19) is None and lip_mirror_perm(21) is None


def _test_cfg(mode="ms_test", pairs=None, num_classes=20):
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    test = {"mode": mode, "scale_search": [0.75, 1.0], "crop_size": [32, 32]}
    if pairs is not None:
        test["flip_swap_pair"] = pairs
    return Configer(config_dict={"data": {"num_classes": num_classes}, "test": test})


def test_check_config_and_flip_swap_pair():
    from contrastiveseg_amd.segmentor.tester import check_config, flip_swap_perm
    for mode in ("ss_test", "ms_test"):
        assert check_config(_test_cfg(mode, LIP_PAIRS))[0] == mode
        assert flip_swap_perm(_test_cfg(mode, LIP_PAIRS)) == LIP_PERM
    assert flip_swap_perm(_test_cfg("ms_test")) is None and flip_swap_perm(_test_cfg("ms_test", [])) is None
    assert flip_swap_perm(_test_cfg("ms_test", [[1, 2], [0, 4], [2, 1]], 5)) == [4, 2, 1, 3, 0]
    with pytest.raises(ValueError, match="is not a permutation"):           # overlapping pairs: channels cannot trade places that way
        check_config(_test_cfg("ms_test", [[1, 2], [2, 3]], 5))
    for mode in ("sscrop_test", "mscrop_test"):
        assert check_config(_test_cfg(mode))[0] == mode                     # the modes themselves stay accepted
        assert check_config(_test_cfg(mode, []))[0] == mode
        with pytest.raises(NotImplementedError, match="test.flip_swap_pair together with test.mode '%s'" % mode):
            check_config(_test_cfg(mode, LIP_PAIRS))
    for pairs in ([[14, 20]], [[-1, 3]], [[19, 19], [0, 25]]):
        with pytest.raises(ValueError, match="test.flip_swap_pair entry .* lies outside the 20 classes"):
            check_config(_test_cfg("ms_test", pairs))
    with pytest.raises(ValueError, match="lies outside the 19 classes"):
        check_config(_test_cfg("ms_test", LIP_PAIRS, 19))
    for pairs in ([[14, 15, 16]], [[14, 1.5]], [14, 15]):
        with pytest.raises(ValueError, match="two class indices"):
            check_config(_test_cfg("ms_test", pairs))


def test_the_lip_configs_load_and_construct_their_transforms():
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUBatchTransform
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tester import check_config, flip_swap_perm, is_ragged
    train = Configer(configs=os.path.join(ROOT, "configs", "lip", "H_48_D_4.json"))
    assert train.get("dataset") == "lip" and train.get("data", "num_classes") == 20
    assert train.get("network", "model_name") == "hrnet_w48_contrast" and train.get("loss", "loss_type") == "contrast_auxce_loss"
    t = GPUBatchTransform(train, "train")
    assert t.aug.seq == ["random_hflip", "resize", "random_resize", "random_crop", "random_brightness"] and not t.aug.canonical
    assert (t.target_w, t.target_h) == (473, 473) and t.lut is None and t.lut_mirrored[:20].tolist() == LIP_PERM
    random.seed(5)
    params, _, target = t.plan_ragged([(300, 500), (473, 473), (640, 480)])
    assert target == (473, 473) and params.shape == (3, 16)
    v = GPUBatchTransform(train, "val")
    assert v.aug.seq == ["resize"] and v.lut_mirrored is None
    assert check_config(train)[0] == "ss_test" and flip_swap_perm(train) is None      # the reference's tester: no swap
    test = Configer(configs=os.path.join(ROOT, "configs", "lip", "H_48_D_4_TEST.json"))
    mode, scales, weights = check_config(test)
    assert mode == "ms_test" and scales == [0.5, 0.75, 1, 1.25, 1.5] and weights is None and is_ragged(test)
    assert test.get("test", "flip_swap_pair") == LIP_PAIRS and flip_swap_perm(test) == LIP_PERM
    assert GPUBatchTransform(test, "train").lut_mirrored[:20].tolist() == LIP_PERM
    GPUBatchTransform(test, "test")


def test_two_flips_with_pairs_that_share_an_id_are_refused():
    """The kernels swap by the parity of the applied flips; a map that is not its own inverse, applied twice, is not the identity."""
    from contrastiveseg_amd.lib.datasets.tools.gpu_aug import GPUAugCompose
    twice = ["random_hflip", "resize", "random_hflip", "random_crop"]
    cfg = _cfg([[1, 2], [2, 3]])
    cfg.get("train_trans")["trans_seq"] = twice
    with pytest.raises(NotImplementedError, match="more than one random_hflip"):
        GPUAugCompose(cfg)
    cfg = _cfg(LIP_PAIRS)
    cfg.get("train_trans")["trans_seq"] = twice
    assert GPUAugCompose(cfg).swap[:20].tolist() == LIP_PERM


def test_trainer_validation_takes_the_lip_branch_on_cpu(monkeypatch):
    """dataset == 'lip': one forward on the batch and its mirror together, the torch composition of the reference (CSEG_VAL_FUSED=0;
    the fused path needs the device), no validation loss. Device half of the model = oracle/cpu_port.py."""
    import torch.nn.functional as F
    from oracle import cpu_port
    cpu_port.install(monkeypatch)
    from contrastiveseg_amd.lib.utils.tools.configer import Configer
    from contrastiveseg_amd.segmentor.tools.data_helper import SyntheticLoader
    from contrastiveseg_amd.segmentor.trainer_contrastive import Trainer
    monkeypatch.setenv("CSEG_VAL_FUSED", "0")
    cfg = Configer(configs=os.path.join(ROOT, "configs", "synthetic", "R_18_D_8_tiny.json"))
    cfg.add(["network", "pretrained"], None)
    cfg.add(["network", "resume"], None)
    cfg.add(["gpu"], None)
    cfg.update(["dataset"], "lip")
    cfg.update(["data", "num_classes"], 20)
    cfg.get("train", "data_transformer")["input_size"] = [64, 48]
    cfg.update(["train", "batch_size"], 2)
    cfg.params_root.pop("checkpoints", None)
    torch.manual_seed(304)
    tr = Trainer(cfg, train_loader=[])
    batches = list(SyntheticLoader(cfg, torch.device("cpu"), length=2, mode="blocky", fixed=False))
    seen = []
    net = tr.seg_net
    forward = net.forward
    monkeypatch.setattr(net, "forward", lambda x, **kw: (seen.append(tuple(x.shape)), forward(x, **kw))[1])
    tr.validate(batches)
    assert seen == [(4, 3, 48, 64)] * 2                    # the batch and its mirror in one pass
    assert tr.val_losses.count == 0                         # no validation loss in this branch
    got = tr.last_val_score.confusion_matrix
    want = torch.zeros(20, 20, dtype=torch.int64)
    net.eval()
    with torch.no_grad():
        for b in batches:
            seg = forward(torch.cat([b["img"], torch.flip(b["img"], [3])], 0), is_eval=True)["seg"]
            assert seg.shape[1] == 20
            rev = seg[2:].index_select(1, torch.tensor(LIP_PERM)).flip(3)
            pred = F.interpolate((seg[:2] + rev) / 2., size=(48, 64), mode="bilinear", align_corners=True).argmax(1)
            t = b["labelmap"]
            want += torch.bincount(20 * t[t >= 0] + pred[t >= 0], minlength=400).reshape(20, 20)
    assert torch.equal(got, want) and int(got.sum()) > 0
    assert cfg.get("performance") == float(tr.last_val_score.get_mean_iou())
