"""Data pipeline of the search (src/data): list-file dataset, augmentations, loaders - numpy / PIL / torch only."""
from .datasets import (CentralCrop, Compose, DepthDataset, DepthResizeScale, Normalise, Pad,  # noqa: F401
                       PascalCustomDataset, RandomCrop, RandomMirror, ResizeScale, ResizeShorter, ToTensor)
from .loaders import create_depth_loaders, create_loaders  # noqa: F401
