"""Mirror of ptt.datasets.augmentor: DataAugmentor (random_world_flip / random_world_rotation / random_world_scaling) on the host.
TrainBatchFeeder applies the same operations on the device, as one composite map per sample (ptt_amd/train_feed.py)."""
from .data_augmentor import DataAugmentor          # noqa: F401
