"""Data-side mirror, limited to what the tracking loop and the training feeder need: ptt.datasets.kitti.kitti_tracking_utils
(the sequential tracking loop's pre/post-processing) and ptt.datasets.augmentor (DataAugmentor's world flip /
rotation / scaling, which ptt_amd.train_feed applies on the device). Dataset loading and IO stay out of scope."""
