from .loss import DiceLoss, IouLoss, MultiLoss, get_loss      # noqa: F401
from .miou import MDiceLoss, MIouLoss, MaskOneHot    # noqa: F401
from .lossm import CrossEntropyLoss, get_mloss       # noqa: F401
