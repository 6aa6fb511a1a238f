// The left/right channel table of a mirrored FLIC heat map: where channel k of the mirror image reads from (augmentation.py:20, applied by
// random_flip as the concat [3,4,5, 0,1,2, 7, 6, 8, 9]): shoulders, elbows and wrists 0-2 <-> 3-5, hips 6 <-> 7, nose and torso in place.
// An involution.  Shared by the training-time flip (augment.hip) and the mirrored test-time evaluation (mirror.hip); usable on host and device.
#pragma once

namespace jcm {

constexpr int kHmFlipChannels = 10;
constexpr int kHmFlipPerm[kHmFlipChannels] = {3, 4, 5, 0, 1, 2, 7, 6, 8, 9};

}  // namespace jcm
