def kitti_tracklets(*args, **kwargs):
    """kitti_scenes.kitti_tracklets; imported on use, so that the host-only readers (kitti_files) load without the device library."""
    from .kitti_scenes import kitti_tracklets as impl
    return impl(*args, **kwargs)
