#pragma once
#include "BamAlignment.h"
namespace BamTools { struct BamReader {}; }
