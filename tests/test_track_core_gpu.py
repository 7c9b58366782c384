"""TrackCore.ready on the GPU: the ONE rule for when the resampling table is built and uploaded again — when something it addresses
moved (the model's input buffers, the crop slots), and only then."""
import numpy as np
import pytest
import torch

from tests.test_online_tracker_gpu import _tracker

pytestmark = pytest.mark.gpu


def test_ready_uploads_the_resampling_table_only_when_its_buffers_moved(dev, monkeypatch):
    from ptt_amd import ops
    from ptt_amd.track_core import TrackCore, resample_table
    tracker = _tracker(dev)
    core = TrackCore(tracker, dev, 2, shape="firstandprevious")
    uploads = []
    real = ops.upload_jobs

    def counted(jobs, out=None):
        if out is core.reg_jobs_dev:
            uploads.append(jobs.copy())
        return real(jobs, out)
    monkeypatch.setattr(ops, "upload_jobs", counted)

    def check(n, what):
        """n uploads so far; the device table is the one built over the buffers the core holds NOW."""
        assert len(uploads) == n, "%s: %d uploads, expected %d" % (what, len(uploads), n)
        torch.cuda.synchronize(dev)
        want = resample_table("firstandprevious", core.out_ptr, core.cnt_ptr, core.cap, core.search.data_ptr(), core.template.data_ptr(),
                              core.info.data_ptr(), core.S, core.T)
        assert core.reg_jobs_dev.cpu().numpy().tobytes() == want.tobytes() == uploads[-1].tobytes(), what

    core.ready(300)
    assert core.graph is not None and core.graph.captures == 1 and core.cap == 300 and tuple(core.crop_out.shape) == (2, 3, 300, 3)
    assert core.search.data_ptr() == core.graph.search.data_ptr() and core.template.data_ptr() == core.graph.template.data_ptr()
    check(1, "first ready")
    graph, slots = core.graph, core.crop_out.data_ptr()
    core.ready(300)
    core.ready(17)                                             # grow-only: a smaller request changes nothing
    assert core.graph is graph and core.crop_out.data_ptr() == slots and core.cap == 300
    check(1, "same cap again")
    keep = core.crop_out                                       # held, so that the new slots cannot land on its address
    core.ready(301)
    assert core.graph is graph and core.cap == 301 and core.crop_out.data_ptr() != keep.data_ptr()
    check(2, "larger cap: the crop slots moved")
    inputs = (core.search.data_ptr(), core.template.data_ptr())
    tracker.load_state_dict(tracker.state_dict())              # the same values, written again: every graph over them is stale
    core.ready(301)
    assert core.graph is not graph and core.graph.captures == 1
    moved = (core.search.data_ptr(), core.template.data_ptr()) != inputs
    check(2 + int(moved), "new graph, inputs %s" % ("moved" if moved else "at the old addresses"))
    core.ready(301)
    check(2 + int(moved), "nothing changed")
    assert np.array_equal(core.reg_jobs, uploads[-1])
