"""Data-side mirror, limited to what the tracking loop and the training feeder need: ptt.datasets.kitti.kitti_tracking_utils
(the sequential tracking loop's pre/post-processing), ptt.datasets.augmentor (DataAugmentor's world flip /
rotation / scaling, which ptt_amd.train_feed applies on the device), and the KITTI tracking files: kitti.kitti_files (calibration,
labels, tracklet grouping, annotation -> box, on the host) and kitti.kitti_scenes (KittiTrackingScenes: a KITTI directory read
once into a SceneStore and handed to the runners, the feeder, fit and OnlineTracker). nuScenes files, the pickle database and
build_dataloader stay out of scope (INTEGRATION.md §3 "KITTI files")."""
