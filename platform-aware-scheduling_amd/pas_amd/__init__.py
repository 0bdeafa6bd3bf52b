"""pas_amd — Python handle on the MI355X-native Platform Aware Scheduling evaluator.

The evaluator itself is lib/libpas.so (HIP kernels for gfx950 + the C-ABI of
include/pas.h); this package loads it with ctypes and adds synthetic workloads.
Importing it loads the library and fails loudly when it has not been built.
"""
from . import _lib
from ._lib import (PAS_OP_EQUALS, PAS_OP_GREATER_THAN, PAS_OP_LESS_THAN, PAS_TAS_FILTER,
                   PAS_TAS_PRIORITIZE, PasError)
from .context import (RULE_DTYPE, Context, gas_annotation_parse, gas_annotation_render,
                      label_patch_json,
                      label_patch_json_batch, make_rules, name_hash, parse_operator,
                      quantity_as_int64, quantity_decimals,
                      quantity_parse_fixed, quantity_to_milli, quantity_to_scaled,
                      quantity_to_wide, w64)

LIB = _lib.load()

__all__ = [
    "Context", "PasError", "RULE_DTYPE", "make_rules", "parse_operator", "quantity_to_milli",
    "quantity_to_scaled", "quantity_to_wide", "quantity_decimals", "quantity_parse_fixed",
    "quantity_as_int64", "name_hash", "gas_annotation_parse", "gas_annotation_render", "w64", "label_patch_json", "label_patch_json_batch", "PAS_OP_LESS_THAN", "PAS_OP_GREATER_THAN", "PAS_OP_EQUALS",
    "PAS_TAS_FILTER", "PAS_TAS_PRIORITIZE", "LIB",
]
