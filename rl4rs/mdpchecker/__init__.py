"""Reference import path of the MDP checker (``rl4rs.mdpchecker.decoder``); the implementation is ``rl4rs_amd.mdpchecker``."""
