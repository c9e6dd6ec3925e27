# Drop this file over lib/test/tracker/ostrack.py of the reference tree:
# the harness imports `lib.test.tracker.ostrack` and calls get_tracker_class().
from vittracker_amd.tracker.ostrack import OSTrack, get_tracker_class  # noqa: F401
