"""lib/network/rtpose_hourglass.py surface -> MI355X implementation (``import network.rtpose_hourglass as hourglass``,
train/train_SH.py:14)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from _rtpose_pkg import module  # noqa: E402

_hg = module("hourglass")
NUM_JOINTS = _hg.NUM_JOINTS
NUM_LIMBS = _hg.NUM_LIMBS
Bottleneck = _hg.Bottleneck
Hourglass = _hg.Hourglass
HourglassNet = _hg.HourglassNet
hg = _hg.hg
