"""The prediction layer, from image files to joints in each image's own pixels, and its one public surface.  One module per stage, each opening with its
part of DESIGN.md 4.16-4.24: images (the letterboxed forward, the zoom pass), clips (frame sequences and the online trackers), render, files; the
names of the motion model the clips share with the engine (../motion.py) are given here too."""
from ..motion import (SEQ_CAMERA_SEARCH, SEQ_EXCLUDE, SEQ_FLOW_MAX, SEQ_FLOW_SEARCH, SEQ_KEYS, SEQ_MODES, SEQ_RADIUS_MAX, SEQ_RHO, SEQ_SIGMA, SEQ_SIGMA_MAX, SEQ_TORSO_SIGMA, seq_fit, seq_m_step,  # noqa: F401
                      camera_shifts, flow_cell_shifts, flow_refs, flow_weights, seq_moment, seq_pose_tau, seq_radius, seq_sigma_of_moment, seq_taps)
from .clips import SEQ_CAMERA_MODES, SEQ_FLOW_CENTRE_MODES, SEQ_FLOW_MODES, SEQ_ZOOM_MODES, ZOOM_MAP, LagTracker, PeopleTracker, SequenceTracker, predict_sequence, predict_sequence_people, predict_sequence_zoom, zoom_window_track  # noqa: F401
from .files import IMAGE_EXTENSIONS, expand_paths, load_image, predictions_document  # noqa: F401
from .images import FIT_SIDE_MAX, FRAME, JOINT_NAMES, STRIDE, ZOOM_TORSO_JOINTS, ZOOM_TORSO_PIXELS, _coords_to_points, predict_images, torso_length, zoom_windows  # noqa: F401
from .render import HEAT_MASK, JOINT_ALPHA, JOINT_RGB, LIMB_ALPHA, NECK, SKELETON, render_images, skeleton_primitives  # noqa: F401
