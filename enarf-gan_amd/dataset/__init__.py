"""The reference's dataset/ package, for the pose prior: dataset.HumanPoseDataset and utils_3d's bone masks, drawn on
the device by libenarf_pose.so (include/enarf_pose.h)."""
