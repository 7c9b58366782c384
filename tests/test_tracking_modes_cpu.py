"""The tracking loop's TEST settings on the CPU: how SHAPE_AGGREGATION / REF_BOX strings are read, and the restated loop
(tests/tracking_modes_ref.py) against fixture G18, the reference's own TrackingEvaluator in all twelve modes."""
import os

import numpy as np
import pytest

from oracle import tracking_ref as TR
from tests import tracking_modes_ref as TM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("text,shape", [
    ("firstandprevious", "firstandprevious"), ("FirstAndPrevious", "firstandprevious"), ("x_firstandprevious_y", "firstandprevious"),
    ("first", "first"), ("FIRST", "first"), ("first_and_previous", "first"), ("previous_first", "first"),
    ("previous", "previous"), ("Previous", "previous"), ("all", "all"), ("ALL", "all"), ("", "all"), ("mean", "all")])
def test_shape_aggregation_is_read_as_the_reference_reads_it(text, shape):
    """prepare_template (eval_tracking_utils.py:187-216): substring tests, FIRSTANDPREVIOUS, then FIRST, then PREVIOUS; anything
    else is `all` — so "first_and_previous" selects `first`, as in the reference."""
    from ptt_amd.tracklet_runner import tracking_modes
    assert tracking_modes(text, "previous_result") == (shape, "previous_result")


@pytest.mark.parametrize("text,ref", [
    ("previous_result", "previous_result"), ("PREVIOUS_RESULT", "previous_result"), ("use_previous_result", "previous_result"),
    ("previous_gt", "previous_gt"), ("Previous_GT", "previous_gt"), ("current_gt", "current_gt"), ("CURRENT_GT", "current_gt")])
def test_ref_box_is_read_as_the_reference_reads_it(text, ref):
    from ptt_amd.tracklet_runner import tracking_modes
    assert tracking_modes("firstandprevious", text) == ("firstandprevious", ref)


@pytest.mark.parametrize("text", ["", "previous", "gt", "result", "current"])
def test_unknown_ref_box_raises(text):
    """prepare_search :161-162 raises for anything but the three settings."""
    from ptt_amd.tracklet_runner import tracking_modes
    with pytest.raises(ValueError):
        tracking_modes("all", text)


def test_runner_defaults_are_the_shipped_settings():
    import inspect
    from ptt_amd.tracklet_runner import TrackletRunner
    sig = inspect.signature(TrackletRunner.__init__)
    assert sig.parameters["shape_aggregation"].default == "firstandprevious"
    assert sig.parameters["ref_box"].default == "previous_result"


def test_G18_restated_loop_equals_the_reference_in_every_mode():
    """tests/tracking_modes_ref.track_modes with G18's stand-in model == the reference's TrackingEvaluator (prepare_search /
    prepare_template / post_process) frame for frame: ref box, result box (a gt-referenced result keeps the gt box's wlh),
    model-point count, search and template clouds, bit for bit — numpy's global generator included (the stand-in's proposals
    send get_box_by_offset down its redraw path)."""
    g = np.load(os.path.join(GOLD, "G18_tracking_modes.npz"))
    infer = TM.standin_model({k[len("param_"):]: g[k] for k in g.files if k.startswith("param_")})
    S, T = (int(v) for v in g["sizes"])
    box = lambda a: TR.RefBox(a[0:3], a[3:6], a[6:10])
    flat = lambda b: np.concatenate([b.center, b.wlh, b.quat.q])
    n_frames = 0
    for t in range(int(g["n_tracklets"])):
        L = int(g["n_frames_%d" % t])
        clouds = [g["cloud_%d_%d" % (t, i)] for i in range(L)]
        gts = [box(g["gt_%d_%d" % (t, i)]) for i in range(L)]
        for shape in g["shapes"]:
            for ref in g["refs"]:
                res, frames = TM.track_modes(clouds, gts, infer, str(shape), str(ref), use_z=True, search_size=S, template_size=T)
                assert len(res) == L
                for i in range(1, L):
                    key = "%d_%s_%s_%d" % (t, shape, ref, i)
                    f = frames[i - 1]
                    np.testing.assert_array_equal(flat(f["ref"]), g["ref_" + key], err_msg=key)
                    np.testing.assert_array_equal(flat(res[i]), g["res_" + key], err_msg=key)
                    assert f["n_model"] == int(g["nmodel_" + key]), key
                    np.testing.assert_array_equal(f["search"], g["search_" + key], err_msg=key)
                    np.testing.assert_array_equal(f["template"], g["template_" + key], err_msg=key)
                    n_frames += 1
    assert n_frames == 12 * (5 + 6)
