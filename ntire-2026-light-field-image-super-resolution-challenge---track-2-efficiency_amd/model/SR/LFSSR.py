"""LFSSR plugin (drop-in for the reference's ``model/SR/LFSSR.py``): ``get_model`` / ``get_loss`` / ``weights_init`` with the
reference's state_dict key names, order and shapes; ``forward`` runs in the gfx950 HIP library through the C ABI
(lfsr_amd.hip_model).  Inference only: scale factors 2 and 4, angRes 2..9; a forward with grad enabled and trainable
parameters raises ``LfsrError``."""
import torch
import torch.nn as nn

from lfsr_amd import capi
from lfsr_amd.hip_model import HipModel, _Holder


class _AltFilter(_Holder):
    # AltFilter.__init__, LFSSR.py:195-201
    def __init__(self):
        super().__init__()
        self.spaconv = nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=1)
        self.angconv = nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=1)


class _Net(_Holder):
    # net2x.__init__ / net4x.__init__, LFSSR.py:51-71,105-139
    def __init__(self, scale, n_layer):
        super().__init__()
        self.conv0 = nn.Conv2d(1, 64, kernel_size=3, stride=1, padding=1)
        for level in ("1", "2")[:1 if scale == 2 else 2]:
            setattr(self, "altblock" + level, nn.Sequential(*[_AltFilter() for _ in range(n_layer)]))
            setattr(self, "fup" + level, nn.Sequential(nn.Conv2d(64, 64 * 4, kernel_size=3, stride=1, padding=1), nn.PixelShuffle(2), nn.ReLU(inplace=True)))
            setattr(self, "res" + level, nn.Conv2d(64, 1, kernel_size=3, stride=1, padding=1))
            setattr(self, "iup" + level, nn.Sequential(nn.Conv2d(1, 4, kernel_size=3, stride=1, padding=1), nn.PixelShuffle(2)))


class get_model(HipModel):
    hip_name = "LFSSR"
    trainable = False
    n_layer = 10              # LFSSR.py:56,111

    def __init__(self, args):
        super().__init__()
        self.angRes = args.angRes_in
        self.factor = args.scale_factor
        if self.factor not in (2, 4):
            raise capi.LfsrError(f"LFSSR: scale factor {self.factor} (the reference has net2x and net4x only)")
        self.net = _Net(self.factor, self.n_layer)

    def _new_runtime(self):
        return capi.LFSSRRuntime(int(self.angRes), int(self.factor), self.n_layer)


def weights_init(m):
    pass


class get_loss(nn.Module):
    # LFSSR.py:219-227
    def __init__(self, args):
        super().__init__()
        self.criterion_Loss = torch.nn.L1Loss()

    def forward(self, SR, HR, criterion_data=[]):
        return self.criterion_Loss(SR, HR)
