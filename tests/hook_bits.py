"""The test hooks of the library flavour with test hooks, by name: the bits of `drt_set_debug_flags` (include/drt_hip.h) as enum Hook of
csrc/drt_device.h lists them - kHookNoGradAtomics is NO_GRAD_ATOMICS here.  The values are ABI; test_host_logic.py holds this list, the
enum and the header's table to each other."""
NO_GRAD_ATOMICS = 1 << 0
PER_LANE_ATOMICS = 1 << 1
NO_OCCUPANCY = 1 << 4
UNTILE_KEEP_SCRATCH = 1 << 6
ATOMIC_GRADIENTS = 1 << 7
TINY_RECORD_STREAMS = 1 << 8
NERF_RECORD_PATH = 1 << 9
REDUCE_NO_FLUSH = 1 << 10
PIPELINE_BATCHES = 1 << 11
NO_QUEUED_TRACER = 1 << 12
FEW_PART_WGS = 1 << 13
SMALL_RECORD_BUDGET = 1 << 14
NO_RECORD_MEMORY = 1 << 18
NO_RECORD_MEMORY_LATER = 1 << 19
NO_PATH_CACHE = 1 << 20
GENERIC_KERNELS = 1 << 21
NO_RAY_SCHEDULE = 1 << 22
NO_SUPERGRID_MASK = 1 << 23
PLAIN_BLOCK_MAP = 1 << 24
NO_HAND_OFF = 1 << 25
NO_HAND_OFF_PRIMAL = 1 << 26
NO_TAIL_OVERLAP = 1 << 28
INDEX_ORDER = 1 << 29
SCHEDULE_SMALL = 1 << 30
WALK_EMPTY_PIXELS = 1 << 31

# the bits that selected the older tracer generations (the per-lane Tracer, the state machine of whole flights, the round-3 supergrid
# kernel): drt_set_debug_flags refuses a word that contains one of them
RETIRED = (1 << 3) | (1 << 5) | (1 << 15) | (1 << 16) | (1 << 27)
