"""RCF edge detector -- host mirror of mdir/components/model/network/rcf.py:21-155 (the rcfngan / rcfgan scenarios' detector,
mdir/examples/iccv23/train/rcfngan.yml:7-11; forward-only, run on the day image and on the generated night image).

Same module attributes and state_dict keys as the reference (64 tensors), so its checkpoints load unchanged.  The four fixed bilinear
deconv kernels are non-persistent buffers built on the CPU (the reference calls ``.cuda()`` on them in ``__init__``, rcf.py:69-72): they
follow ``.to(device)`` and are not part of the state.  On a HIP device the forward is ``engine.build_rcf``'s graph."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hipbacked import HipBacked


def _make_bilinear_weights(size, num_channels):
    """rcf.py:77-92 (float64 filter, stored in a float32 tensor)"""
    factor = (size + 1) // 2
    center = factor - 1 if size % 2 == 1 else factor - 0.5
    og = np.ogrid[:size, :size]
    filt = torch.from_numpy((1 - abs(og[0] - center) / factor) * (1 - abs(og[1] - center) / factor))
    w = torch.zeros(num_channels, num_channels, size, size)
    for i in range(num_channels):
        w[i, i] = filt
    return w


class RCF(HipBacked, nn.Module):
    meta = {"in_channels": 3, "out_channels": 1}
    _disable_graphviz = True
    #: on a HIP device the wrapper chain hands its trailing per-channel input wrappers over as ``input_transform``
    accepts_input_transform = True

    def __init__(self, pretrained=None):
        super().__init__()
        chans = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
        names = ["conv%d_%d" % (b, i) for b, n in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3)) for i in range(1, n + 1)]
        for name, (cin, cout) in zip(names, chans):
            dil = 2 if name.startswith("conv5") else 1
            setattr(self, name, nn.Conv2d(cin, cout, 3, padding=dil, dilation=dil))
        self.pool1 = nn.MaxPool2d(2, stride=2, ceil_mode=True)
        self.pool2 = nn.MaxPool2d(2, stride=2, ceil_mode=True)
        self.pool3 = nn.MaxPool2d(2, stride=2, ceil_mode=True)
        self.pool4 = nn.MaxPool2d(2, stride=1, ceil_mode=True)
        self.act = nn.ReLU(inplace=True)
        for name, (_, cout) in zip(names, chans):
            setattr(self, name + "_down", nn.Conv2d(cout, 21, 1))
        for k in range(1, 6):
            setattr(self, "score_dsn%d" % k, nn.Conv2d(21, 1, 1))
        self.score_fuse = nn.Conv2d(5, 1, 1)
        for k, size in ((2, 4), (3, 8), (4, 16), (5, 16)):
            self.register_buffer("weight_deconv%d" % k, _make_bilinear_weights(size, 1), persistent=False)
        if pretrained:
            from ....tools.utils import fs_open
            with fs_open(pretrained) as handle:
                self.load_state_dict(torch.load(handle, map_location="cpu"))

    @staticmethod
    def _crop(data, img_h, img_w, crop_h, crop_w):
        """rcf.py:95-99"""
        _, _, h, w = data.size()
        assert img_h <= h and img_w <= w
        return data[:, :, crop_h:crop_h + img_h, crop_w:crop_w + img_w]

    def forward(self, x, no_sigmoid=False, features=False, interpolate=False, input_transform=None):
        """``features`` / ``interpolate`` are accepted and ignored, as in the reference.  ``input_transform``: per-channel (perm, scale, shift)
        applied inside the HIP input-pack kernel, passed per call by Compose (components/data/wrapper.py, _fold_input_wrappers)"""
        if input_transform is not None and self._hip_device().type != "cuda":
            raise ValueError("input_transform is a HIP-path argument")
        if self._hip_device().type == "cuda":
            from .... import engine
            self._hip_check_inference()
            prec = self._hip_precision()
            tr = input_transform
            net = self._hip_net(("rcf", bool(no_sigmoid), prec, tr),
                                lambda sd, dev: engine.build_rcf(sd, dev, sigmoid=not no_sigmoid, precision=prec, perm=None if tr is None else list(tr[0]),
                                                                 in_affine=None if tr is None else (list(tr[1]), list(tr[2]))))
            return net.forward(x)[net.out_slot]
        img_h, img_w = x.shape[2], x.shape[3]
        act = self.act
        conv1_1 = act(self.conv1_1(x))
        conv1_2 = act(self.conv1_2(conv1_1))
        conv2_1 = act(self.conv2_1(self.pool1(conv1_2)))
        conv2_2 = act(self.conv2_2(conv2_1))
        conv3_1 = act(self.conv3_1(self.pool2(conv2_2)))
        conv3_2 = act(self.conv3_2(conv3_1))
        conv3_3 = act(self.conv3_3(conv3_2))
        conv4_1 = act(self.conv4_1(self.pool3(conv3_3)))
        conv4_2 = act(self.conv4_2(conv4_1))
        conv4_3 = act(self.conv4_3(conv4_2))
        conv5_1 = act(self.conv5_1(self.pool4(conv4_3)))
        conv5_2 = act(self.conv5_2(conv5_1))
        conv5_3 = act(self.conv5_3(conv5_2))
        out1 = self.score_dsn1(self.conv1_1_down(conv1_1) + self.conv1_2_down(conv1_2))
        out2 = self.score_dsn2(self.conv2_1_down(conv2_1) + self.conv2_2_down(conv2_2))
        out3 = self.score_dsn3(self.conv3_1_down(conv3_1) + self.conv3_2_down(conv3_2) + self.conv3_3_down(conv3_3))
        out4 = self.score_dsn4(self.conv4_1_down(conv4_1) + self.conv4_2_down(conv4_2) + self.conv4_3_down(conv4_3))
        out5 = self.score_dsn5(self.conv5_1_down(conv5_1) + self.conv5_2_down(conv5_2) + self.conv5_3_down(conv5_3))
        out2 = self._crop(F.conv_transpose2d(out2, self.weight_deconv2, stride=2), img_h, img_w, 1, 1)
        out3 = self._crop(F.conv_transpose2d(out3, self.weight_deconv3, stride=4), img_h, img_w, 2, 2)
        out4 = self._crop(F.conv_transpose2d(out4, self.weight_deconv4, stride=8), img_h, img_w, 4, 4)
        out5 = self._crop(F.conv_transpose2d(out5, self.weight_deconv5, stride=8), img_h, img_w, 0, 0)
        fuse = self.score_fuse(torch.cat((out1, out2, out3, out4, out5), dim=1))
        return fuse if no_sigmoid else torch.sigmoid(fuse)
