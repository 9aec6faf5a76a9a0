"""metacherchant_amd -- MI355X-native implementation of MetaCherchant's environment-finder hot path.

The product is libmcgpu.so (hand-written HIP for gfx950 behind the C ABI of include/mcgpu.h) plus
the C++ host tool; this package only binds it for tests, benchmarks and multi-GPU orchestration.
"""
from . import native  # noqa: F401
from .native import KEY_FNV1A, KEY_PACKED, KEY_POLY, Context, McError, seq_coverage, seq_coverage_dev  # noqa: F401
from .native import kmer_presence, kmer_presence_dev, reads_in_set, reads_in_set_dev  # noqa: F401
from .native import components, components_dev  # noqa: F401
from .native import unitigs, unitigs_dev  # noqa: F401
from .native import env_join, env_join_dev  # noqa: F401
from .native import trim_paths, trim_paths_dev  # noqa: F401
from .native import walk_order, walk_order_dev, WALK_ORDER_WIDE_ONLY, WALK_ORDER_NARROW_8  # noqa: F401
from .native import tokenize_whole, tokenize_whole_dev, reads_append_dev  # noqa: F401
from .native import render_fastq, render_fastq_dev, render_fastq_bound  # noqa: F401

__all__ = ["native", "Context", "McError", "KEY_PACKED", "KEY_POLY", "KEY_FNV1A", "seq_coverage", "seq_coverage_dev", "kmer_presence",
           "kmer_presence_dev", "reads_in_set", "reads_in_set_dev", "components", "components_dev", "unitigs", "unitigs_dev",
           "env_join", "env_join_dev", "trim_paths", "trim_paths_dev", "walk_order", "walk_order_dev", "WALK_ORDER_WIDE_ONLY", "WALK_ORDER_NARROW_8", "tokenize_whole", "tokenize_whole_dev", "reads_append_dev",
           "render_fastq", "render_fastq_dev", "render_fastq_bound"]
