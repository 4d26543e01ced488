// The head sets of the pack checkers (pack_plan_check.cpp, pack_host_check.cpp) come from the command line as
// name:channels,... (one argument per set; none: the production set).  Plain C++.
#pragma once

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/sfa_hip.h"

static const char* const kProductionSet = "hm_cen:3,cen_offset:2,direction:2,z_coor:1,dim:3";

static bool parse_set(const char* text, sfa_arch* a) {
  memset(a, 0, sizeof *a);
  a->num_layers = 18;
  a->head_conv = 64;
  std::string s(text);
  size_t pos = 0;
  while (pos < s.size()) {
    size_t end = s.find(',', pos);
    if (end == std::string::npos) end = s.size();
    const std::string item = s.substr(pos, end - pos);
    const size_t colon = item.find(':');
    if (colon == std::string::npos || colon == 0 || colon >= 32 || a->num_heads >= SFA_MAX_HEADS) return false;
    memcpy(a->head_names[a->num_heads], item.c_str(), colon);
    a->head_channels[a->num_heads] = atoi(item.c_str() + colon + 1);
    if (a->head_channels[a->num_heads] < 1 || a->head_channels[a->num_heads] > 4) return false;
    ++a->num_heads;
    pos = end + 1;
  }
  return a->num_heads >= 1;
}

static std::vector<std::string> sets_of(int argc, char** argv) {
  std::vector<std::string> sets;
  for (int i = 1; i < argc; ++i) sets.push_back(argv[i]);
  if (sets.empty()) sets.push_back(kProductionSet);
  return sets;
}
