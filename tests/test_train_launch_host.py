"""apps/train_SuRS.main() as the launcher of a data-parallel run, without a device: --world_size N and no --rank starts N child
processes running main(... --rank r) and waits; ranks that fail - here at init_process_group, on an unknown backend, before anything
touches a GPU - end the run with SystemExit instead of leaving the parent waiting.  (The run that succeeds is a GPU test:
tests/test_gpu_train_dist.py, mode `launch`.)"""
import socket

import pytest


def test_main_starts_the_ranks_and_reports_their_failure(capfd):
    from surs_amd.apps import train_SuRS
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with pytest.raises(SystemExit) as e:
        train_SuRS.main(["--world_size", "2", "--dist_backend", "no_such_backend", "--dist_url", "tcp://127.0.0.1:%d" % port,
                         "--num_epoch", "0"])
    assert "a rank ended with status" in str(e.value)
    err = capfd.readouterr().err
    assert "no_such_backend" in err                     # (the children's own traceback: they did parse the flags and reach the group)


def test_a_rank_needs_its_rank():
    """train() itself never starts processes: --world_size above 1 without a valid --rank is refused before anything else happens."""
    from surs_amd import options
    from surs_amd.apps import train_SuRS
    opt = options.BaseOptions().parse(["--world_size", "2"])
    with pytest.raises(ValueError, match="--rank"):
        train_SuRS.train(opt)
