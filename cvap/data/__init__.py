from vipant_amd.data import *  # noqa: F401,F403
