"""Data pipeline of the search (src/data): list-file dataset, augmentations, loaders - numpy / PIL / torch only."""
from .datasets import (CentralCrop, ColourJitter, Compose, DepthDataset, DepthResizeScale, Normalise,  # noqa: F401
                       Pad, PascalCustomDataset, RandomCrop, RandomMirror, ResizeScale, ResizeShorter, ToTensor)
from .loaders import create_depth_loaders, create_loaders  # noqa: F401
