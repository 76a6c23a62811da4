"""The runner's side of the fg-size, bg > fg and empty-outside-box terms, without a device:
the flags and their defaults (dlib/configure/config.py:451-472, 392), when the teacher runs
(train_wsol.py:758-766) and every refused configuration."""
import pytest

from tcam_wsol_video_amd import runner


def _args(*argv):
    return runner.parser(train=True).parse_args(list(argv))


def test_flags_and_defaults():
    a = _args()
    for t in ("size_bg_g_fg_tc", "sizefg_tmp_tc", "empty_out_bb_tc"):
        assert getattr(a, t) is False and getattr(a, t + "_lambda") == 1.0
        assert getattr(a, t + "_start_ep") == 0 and getattr(a, t + "_end_ep") == -1
    assert a.sizefg_tmp_tc_eps == 0.001 and a.sizefg_tmp_tc_knn == 0
    assert a.sizefg_tmp_tc_knn_mode == "instant" and a.sl_tc_epoch_switch_to_sl == -1
    a = _args("--size_bg_g_fg_tc", "True", "--size_bg_g_fg_tc_lambda", "0.5",
              "--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_eps", "0.01", "--sizefg_tmp_tc_start_ep",
              "3", "--empty_out_bb_tc", "True", "--empty_out_bb_tc_end_ep", "7",
              "--sl_tc_epoch_switch_to_sl", "2")
    assert a.size_bg_g_fg_tc and a.sizefg_tmp_tc and a.empty_out_bb_tc
    assert (a.size_bg_g_fg_tc_lambda, a.sizefg_tmp_tc_eps, a.sizefg_tmp_tc_start_ep,
            a.empty_out_bb_tc_end_ep, a.sl_tc_epoch_switch_to_sl) == (0.5, 0.01, 3, 7, 2)
    runner.check_term_config(_args())          # the defaults pass


def test_teacher_runs_when_the_reference_runs_it():
    a = _args("--sl_tc_epoch_switch_to_sl", "3")
    assert [runner.teacher_runs(a, e) for e in (1, 2, 3, 4)] == [False, False, True, True]
    assert not runner.teacher_runs(_args(), 5)                        # -1: never
    a = _args("--empty_out_bb_tc", "True", "--empty_out_bb_tc_start_ep", "2")
    assert [runner.teacher_runs(a, e) for e in (1, 2, 3)] == [False, True, True]
    # only while the self-learning term is on
    a = _args("--sl_tc_epoch_switch_to_sl", "0", "--sl_tc_end_ep", "2")
    assert [runner.teacher_runs(a, e) for e in (1, 2, 3)] == [True, True, False]
    assert not runner.teacher_runs(_args("--sl_tc", "False", "--sl_tc_epoch_switch_to_sl", "0"), 1)


@pytest.mark.parametrize("argv,rule", [
    (["--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_knn_mode", "before",
      "--sl_tc_epoch_switch_to_sl", "0"], "parseit.py:923-924"),
    (["--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_knn", "2", "--sl_tc_epoch_switch_to_sl", "0"],
     "parseit.py:926-928"),
    (["--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_eps", "-0.1", "--sl_tc_epoch_switch_to_sl",
      "0"], "set_eps"),
    # the teacher never runs: fg_size would be None
    (["--sizefg_tmp_tc", "True"], "fg_size would be None"),
    # the teacher starts in epoch 3, the term in epoch 0
    (["--sizefg_tmp_tc", "True", "--sl_tc_epoch_switch_to_sl", "3", "--max_epochs", "4"],
     "fg_size would be None"),
    # self-learning (hence the teacher) stops before the term does
    (["--empty_out_bb_tc", "True", "--sl_tc_end_ep", "1", "--max_epochs", "2"],
     "msk_bbox would be None"),
    (["--empty_out_bb_tc", "True", "--sl_tc", "False"], "msk_bbox would be None"),
])
def test_refused_configurations(argv, rule):
    with pytest.raises(SystemExit) as e:
        runner.check_term_config(_args(*argv))
    assert rule in str(e.value)


@pytest.mark.parametrize("argv", [
    ["--size_bg_g_fg_tc", "True"],                                   # needs no teacher
    ["--empty_out_bb_tc", "True", "--max_epochs", "3"],              # starts the teacher itself
    ["--sizefg_tmp_tc", "True", "--sl_tc_epoch_switch_to_sl", "0", "--max_epochs", "3"],
    ["--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_start_ep", "3", "--sl_tc_epoch_switch_to_sl",
     "3", "--max_epochs", "5"],
    ["--sizefg_tmp_tc", "True", "--sizefg_tmp_tc_knn", "2", "--sizefg_tmp_tc_knn_mode", "before",
     "--sl_tc_epoch_switch_to_sl", "0"],
])
def test_accepted_configurations(argv):
    runner.check_term_config(_args(*argv))
