// pqgpu_rowgroup_host.cpp — host half of the row-group dictionary filter (include/pqgpu.h, "row-group
// dictionary filter"): pqg_chunk_has_non_dictionary_pages, and pqg::rowgroup_bind: the refusals
// pqg_filter_row_groups makes before a launch, the per-(row group, slot) device table with the "usable"
// rule of DictionaryFilter.expandDictionary, and the flat work list of k_rg_any. The row-group form of the
// program image is built with the filter (pqgpu_filter_host.cpp: pqg_filter::rg_image).
// Plain C++ with no HIP in it, so that it also builds alone under the sanitizers
// (tests/c/rowgroup_sanitize.cpp).
#include <algorithm>
#include <new>

#include "pqgpu_rowgroup.h"

namespace {

// parquet-format Encoding and PageType values (include/pqgpu.h: pqg_encoding, pqg_page_type)
constexpr int32_t kPlainDictionary = 2, kRle = 3, kBitPacked = 4, kRleDictionary = 8;
constexpr int32_t kDataPage = 0, kDataPageV2 = 3;

bool remove_all(std::vector<int32_t>* set, int32_t v) {
  const auto end = std::remove(set->begin(), set->end(), v);
  const bool had = end != set->end();
  set->erase(end, set->end());
  return had;
}

// expandDictionary's switch (DictionaryFilter.java:102-124): BOOLEAN and INT96 return null
bool decodable(int type) {
  return type == PQG_INT32 || type == PQG_INT64 || type == PQG_FLOAT || type == PQG_DOUBLE || type == PQG_BYTE_ARRAY ||
         type == PQG_FIXED_LEN_BYTE_ARRAY;
}

}  // namespace

extern "C" int pqg_chunk_has_non_dictionary_pages(const pqg_page_encoding_stat* stats, int n_stats, const int32_t* encodings,
                                                  int n_encodings) {
  if (n_stats >= 0) {
    // convertEncodingStats: the data pages' encodings, whatever their counts; then
    // EncodingStats.hasNonDictionaryEncodedPages on that set
    std::vector<int32_t> data;
    for (int i = 0; stats && i < n_stats; i++)
      if (stats[i].page_type == kDataPage || stats[i].page_type == kDataPageV2) data.push_back(stats[i].encoding);
    if (data.empty()) return 0;
    if (!remove_all(&data, kRleDictionary) && !remove_all(&data, kPlainDictionary)) return 1;  // no dictionary encoding
    return data.empty() ? 0 : 1;
  }
  std::vector<int32_t> set;
  for (int i = 0; encodings && i < n_encodings; i++) set.push_back(encodings[i]);
  if (!remove_all(&set, kPlainDictionary)) return 1;  // not dictionary-encoded, or RLE_DICTIONARY without stats
  remove_all(&set, kRle);
  remove_all(&set, kBitPacked);
  return set.empty() ? 0 : 1;
}

namespace pqg {

static int bind(const pqg_filter* filter, const pqg_rowgroup_column* cols, int n_cols, uint64_t n_row_groups,
                RgPlan* plan) {
  if (!filter || !plan || n_cols != (int)filter->column_types.size()) return PQG_ERR_INVALID_ARG;
  if (n_row_groups > RG_MAX_GROUPS || (n_row_groups && n_cols > 0 && !cols)) return PQG_ERR_INVALID_ARG;
  const uint32_t n_slots = (uint32_t)filter->slot_column.size();
  plan->n_slots = n_slots;
  plan->n_nodes = (uint32_t)filter->program.size();
  plan->cols.clear();
  plan->items.clear();
  // a slot gives k_rg_any work when one of its leaves compares with a value
  bool compares[PQG_FILTER_MAX_NODES] = {};
  for (const pqg_filter_node& nd : filter->program) {
    if (nd.op > PQG_FILTER_NOTIN || (nd.flags & PQG_FILTER_NULL_LITERAL)) continue;
    const size_t s = (size_t)(std::find(filter->slot_column.begin(), filter->slot_column.end(), nd.column) -
                              filter->slot_column.begin());
    if (s < n_slots) compares[s] = true;
  }
  plan->cols.resize((size_t)n_row_groups * n_slots);
  constexpr uint32_t known = PQG_RG_MISSING | PQG_RG_NO_DICTIONARY | PQG_RG_NON_DICT_PAGES | PQG_RG_MAY_CONTAIN_NULL;
  uint64_t n_items = 0;
  for (uint64_t g = 0; g < n_row_groups; g++)
    for (uint32_t s = 0; s < n_slots; s++) {
      const int col = filter->slot_column[s];
      const pqg_rowgroup_column& c = cols[g * (uint64_t)n_cols + (uint64_t)col];
      if (c.reserved || c.dict.reserved || (c.flags & ~known)) return PQG_ERR_INVALID_ARG;
      const int type = filter->column_types[(size_t)col];
      const bool usable =
          !(c.flags & (PQG_RG_MISSING | PQG_RG_NO_DICTIONARY | PQG_RG_NON_DICT_PAGES)) && decodable(type);
      RgColDev& d = plan->cols[(size_t)(g * n_slots + s)];
      d.values = nullptr;
      d.binary = nullptr;
      d.n_entries = usable ? c.dict.n_entries : 0u;
      d.flags = c.flags | (usable ? RG_USABLE : 0u);
      if (!usable || !d.n_entries) continue;
      if (!c.dict.values || (type == PQG_BYTE_ARRAY && !c.dict.binary_data)) return PQG_ERR_INVALID_ARG;
      d.values = c.dict.values;
      d.binary = c.dict.binary_data;
      if (compares[s]) n_items += ((uint64_t)d.n_entries + RG_TILE - 1) / RG_TILE;
    }
  if (n_items > RG_MAX_ITEMS) return PQG_ERR_INVALID_ARG;
  // the work list: a (row group, slot)'s tiles stand together, row groups ascending
  plan->items.reserve((size_t)n_items);
  for (uint64_t g = 0; g < n_row_groups; g++)
    for (uint32_t s = 0; s < n_slots; s++) {
      const RgColDev& d = plan->cols[(size_t)(g * n_slots + s)];
      if (!compares[s] || !d.values) continue;
      const uint32_t tiles = (uint32_t)(((uint64_t)d.n_entries + RG_TILE - 1) / RG_TILE);
      for (uint32_t t = 0; t < tiles; t++) plan->items.push_back(RgItem{(uint32_t)g, (s << 24) | t});
    }
  return PQG_OK;
}

int rowgroup_bind(const pqg_filter* filter, const pqg_rowgroup_column* cols, int n_cols, uint64_t n_row_groups,
                  RgPlan* plan) {
  try {
    return bind(filter, cols, n_cols, n_row_groups, plan);
  } catch (const std::bad_alloc&) {  // tables the host cannot hold
    return PQG_ERR_INVALID_ARG;
  }
}

}  // namespace pqg
