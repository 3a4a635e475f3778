"""MI355X-native batched ABR environment + MPC lookahead.

Importing the package loads the HIP library eagerly; if it has not been built
the import fails (there is no CPU fallback).
"""
from . import _lib
from . import advantage
from .advantage import gae
from .datamodel import MPD, Chunk, ChunkInfo, NetworkInfo, QOEMetric
from .env import BatchedABREnv, obs_dict, pack_traces
from .episodes import EpisodeSampler
from .expert import LookaheadExpert
from .fastmpc import FastMPCController
from .ledger import EpisodeLedger
from .quality import EpisodeQuality
from .mpc import BatchedMPCController, EnvPlayer
from .planner import ForecastMPCController
from .policy import PolicyController, PolicyPopulation, RecurrentPolicyController, RecurrentPolicyPopulation
from .search import HindsightSearch
from .rules import BolaController, BufferBasedController, RateBasedController
from .sharding import ShardedABREnv, ShardStep
from .speed import LatencySpeedController
from .simulator import Simulator
from .tracesynth import TraceModel, synth_traces
from .traces import (load_mpd_file, load_network_info, load_trace_file, save_mpd_file,
                     save_trace_file)

_lib.lib()   # fail loudly at import time when libabr_hip.so is missing

__all__ = ["MPD", "Chunk", "ChunkInfo", "NetworkInfo", "QOEMetric", "BatchedABREnv",
           "BatchedMPCController", "EnvPlayer", "FastMPCController", "PolicyController", "PolicyPopulation", "RecurrentPolicyController", "RecurrentPolicyPopulation", "BufferBasedController", "RateBasedController", "BolaController", "obs_dict", "pack_traces", "Simulator", "ShardedABREnv", "ShardStep", "LatencySpeedController",
           "HindsightSearch", "LookaheadExpert", "ForecastMPCController", "EpisodeSampler", "EpisodeLedger", "EpisodeQuality", "advantage", "gae", "TraceModel", "synth_traces",
           "load_trace_file", "load_network_info", "load_mpd_file", "save_trace_file",
           "save_mpd_file"]
